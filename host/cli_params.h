// The command line of host/cellector: load_params (main.rs:629-677, params.yml) and the extension options, from ONE table.
// A row of options() names an option, the kind of its value, the Params field it fills, what it requires, whether it is
// one-GPU-only and its paragraph of --help; the known-name check, the help text, the value parse and the two families of
// refusals are loops over the rows.  Relations between two options that are no plain "requires" follow as ordinary code.
#pragma once
#include <cmath>
#include <map>
#include <optional>
#include <string>
#include <variant>
#include <vector>

#include "host_text.h"

struct Params {
    std::string ref_mtx, alt_mtx, barcodes, output_directory;
    std::optional<std::string> ground_truth, vcf;
    uint64_t min_alt = 4, min_ref = 4, min_alleles_posterior = 5, min_loci_used = 30;
    double posterior_threshold = 0.999, interquartile_range_multiple = 5.0;
    std::optional<double> expected_percent_minority;  // parsed, never used (quirk Q2)
    int device = -1;                                   // extension: ONE GPU to run on
    std::vector<int> devices;                          // extension: the GPUs to shard the cells over (default: GPU 0)
    bool devices_auto = false;                         // --devices auto: as many visible GPUs as the input can feed
    bool one_gpu() const { return !devices_auto && devices.size() <= 1; }
    bool resolve_near_ties = false;                    // extension: option resolve_ties (single GPU)
    int resolve_assignments = 0;                       // extension: options resolve_ties + resolve_posteriors = 1 (true) / 2 (all)
    bool zscore = false;                               // extension: option normalization = 1 (main.rs:317-318)
    bool locus_expected = false;                       // extension: option locus_moments = 1 (the sums main.rs:394 meant to form)
    std::optional<std::string> initial_minority;       // extension: barcodes of the initial exclusion set (main.rs:37 starts from none)
    std::optional<std::string> cell_detail;            // extension: barcodes whose per-locus records go to cell_detail.tsv (main.rs:176's TODO)
    std::optional<std::string> cells;                  // extension: run on these barcodes only (cellector_restage; combiner main.rs:257-280's mask)
    std::optional<double> downsample_rate;             // extension: probability that a read is removed (combiner's --downsample_rate, main.rs:83-88)
    uint64_t seed = 4;                                 // ... and its --seed
    bool restage() const { return cells || downsample_rate; }
    // extension: a second dataset merged in on the GPU (cellector_combine; the combiner's --alt2 / --ref2 / --barcodes2 and, for
    // --mix_cells, its barcode mask) with the identity locus map: both datasets come from the same variant VCF
    std::optional<std::string> mix_alt, mix_ref, mix_barcodes, mix_cells;
    bool mix() const { return mix_alt.has_value(); }
    // extension: synthetic doublets of the run's own cells, made on the GPU after everything else (cellector_add_doublets; what
    // combiner/src/main.rs:43 announces), thinned with their own rate and the shared --seed
    std::optional<std::string> doublets;
    double doublet_downsample_rate = 0.0;
    // extension: K-genotype class scoring after the ordinary run (cellector_class_posteriors / cellector_refine_classes; one GPU)
    std::optional<std::string> classes;               // barcode<TAB>label, at most 16 distinct labels
    uint64_t refine_classes = 0;                       // hard-EM steps at most (0: score the given labelling only)
    bool class_doublets = false;                       // the pairs' doublet classes beside them (cellector_class_doublets)
    bool class_genotypes = false;                      // cellector_classes.vcf: the classes' genotypes (cellector_class_genotypes)
    // extension: K genotype clusters without labels after the ordinary run (cellector_cluster; one GPU)
    uint64_t cluster = 0;                              // K (0: off)
    uint64_t cluster_restarts = 0;                     // R (0: min(16, 64 / K))
    bool cluster_mask_loop = false;                    // --cluster_mask loop: the loci the loop's last iteration used (all: every used locus)
    // extension: donor demultiplexing after the ordinary run (cellector_donor_posteriors / cellector_match_donors; one GPU)
    std::optional<std::string> donors;                 // the donors' genotypes, a VCF with one sample column per donor (needs --vcf)
    double donor_error = 0.01, donor_ambient = 0.03, donor_doublet_rate = 0.1;
    // extension: a panel of up to 4096 genotyped donors in front of the donor pass (cellector_donor_panel); the donors it finds
    // present are the donors of the pass
    uint64_t donor_panel = 0;                          // 0 = off; else the shortlist: the pairs of a cell are its anchor with its M best singlets
    uint64_t donor_panel_min_cells = 1;                // a donor is present with this many status-0 cells
    // extension: the pool's ambient fraction measured from the donor pass' singlets (cellector_estimate_ambient)
    std::string donor_field = "GT";                    // GT: hard calls; GP, GL, PL: the donors' genotype weights (cellector_donor_posteriors_gp)
    int estimate_ambient = 0;                          // 0 = off, 1 = true: report it, 2 = apply: and score the donors again with it
    // extension: the fit of every cell's called hypothesis, and the cells no genotyped donor explains (cellector_donor_fit)
    bool donor_fit = false;
    std::optional<double> donor_fit_iqr;               // the multiple of the iqr below the lower quartile (default: the library's, 3)
    // extension: the mixing share of every called doublet's two donors (cellector_donor_pair_fractions)
    bool doublet_fraction = false;
    std::optional<double> doublet_min_fraction;        // a share within this of 1 or 0 leans to one donor (default: the library's, 0.1)
    // extension: the donors' genotypes from the reads of the cells called for them (cellector_donor_genotypes)
    int donor_genotypes = 0;                           // 0 = off, 1 = true: write them, 2 = apply: and score the donors again with them
    // extension: how -a / -r (and --mix_alt / --mix_ref) belong together: 0 = zipped line by line (the reference's reading),
    // CELLECTOR_JOIN_REF = joined by (locus, cell), CELLECTOR_JOIN_DEPTH = likewise, -r holding alt + ref (cellector_ingest_mtx_joined)
    int matrix_pair = 0;
    // extension: the staged matrix, after every flag that changes it, as an mtx text pair in the output directory
    // (cellector_write_mtx): 0 = off, 1 + CELLECTOR_WRITE_ALIGNED / _SPARSE / _DEPTH
    int write_matrices = 0;
    bool write_matrices_gz = false;                    // ... as .mtx.gz: BGZF compressed on the GPU (cellector_write_mtx_bgzf)
    // extension: a block-compressed (BGZF) -a / -r / --mix_alt / --mix_ref is inflated on the GPU, not on the host (option gz_device)
    bool gz_device = false;
};

// ---- one row of the option table --------------------------------------------------------------------------------
enum class Kind {
    PATH,        // any text
    USIZE,       // an unsigned integer (parse_usize), within `range` if the row has one
    F64,         // a number (parse_f64), within `range` if the row has one
    WORD,        // one of `words`; anything else is the reference's unwrap() panic: exit 101
    WORD_USAGE,  // one of `words`; anything else is a usage error: exit 1
    DEVICES,     // a,b,... or auto
};
struct Range { double lo, hi; bool lo_open, hi_open; };
using Field = std::variant<std::monostate, std::string Params::*, std::optional<std::string> Params::*, uint64_t Params::*, int Params::*,
                           bool Params::*, double Params::*, std::optional<double> Params::*>;
struct Opt {
    const char *name;
    char short_name;  // 0: none
    Kind kind;
    Field field;      // std::string takes the text, uint64_t / double the number, bool / int a WORD's place in `words`
    const char *shown = nullptr;     // the option as the refusals quote it, "--cluster <K>" or "--donor_fit true"
    const char *words = nullptr;     // WORD: the words, '|' between them, in the order of their values 0, 1, ...
    std::optional<Range> range;      // USIZE, F64: the values accepted ...
    const char *expected = nullptr;  // ... and the end of the refusal, "expected a number in [0, 1]" or "expected true or false"
    const char *needs = nullptr;     // the name of the option this one requires
    const char *one_gpu = nullptr;   // one-GPU-only: the option as that refusal quotes it (%s: the value given)
    const char *help = nullptr;      // its paragraph of --help, whole lines

    Opt(const char *name_, char short_name_, Kind kind_, Field field_) : name(name_), short_name(short_name_), kind(kind_), field(field_) {}
    Opt &&as(const char *s) && { shown = s; return std::move(*this); }
    Opt &&one_of(const char *w, const char *e) && { words = w; expected = e; return std::move(*this); }
    Opt &&within(Range r, const char *e) && { range = r; expected = e; return std::move(*this); }
    Opt &&requires_option(const char *n) && { needs = n; return std::move(*this); }
    Opt &&on_one_gpu(const char *s) && { one_gpu = s; return std::move(*this); }
    Opt &&paragraph(const char *h) && { help = h; return std::move(*this); }
};

inline const std::vector<Opt> &options()
{
    using P = Params;
    constexpr Range RATE{0.0, 1.0, false, false};
    static const std::vector<Opt> table = {
        Opt("alt", 'a', Kind::PATH, &P::alt_mtx).paragraph(
            "    -a, --alt <alt>                                                    alt.mtx matrix from vartrix\n"),
        Opt("barcodes", 'b', Kind::PATH, &P::barcodes).paragraph(
            "    -b, --barcodes <barcodes>                                          cell barcodes\n"),
        Opt("expected_percent_minority", 0, Kind::F64, &P::expected_percent_minority).paragraph(
            "        --expected_percent_minority <expected_percent_minority>        percent of cells expected to come from the minority genotype\n"),
        Opt("ground_truth", 'g', Kind::PATH, &P::ground_truth).paragraph(
            "    -g, --ground_truth <ground_truth>                                  cell hashing assignments or other ground truth\n"),
        Opt("interquartile_range_multiple", 0, Kind::F64, &P::interquartile_range_multiple).paragraph(
            "        --interquartile_range_multiple <interquartile_range_multiple>  IQR multiples below the 25th percentile for the outlier threshold\n"),
        Opt("min_alleles_posterior", 0, Kind::USIZE, &P::min_alleles_posterior).paragraph(
            "        --min_alleles_posterior <min_alleles_posterior>                minimum alleles per distribution for the posterior calculation\n"),
        Opt("min_alt", 0, Kind::USIZE, &P::min_alt).paragraph(
            "        --min_alt <min_alt>                                            minimum number of cells containing the alt allele (default 4)\n"),
        Opt("min_loci_for_assignment", 0, Kind::USIZE, &P::min_loci_used).paragraph(
            "        --min_loci_for_assignment <min_loci_for_assignment>            minimum loci to assign a cell (default 30)\n"),
        Opt("min_ref", 0, Kind::USIZE, &P::min_ref).paragraph(
            "        --min_ref <min_ref>                                            minimum number of cells containing the ref allele (default 4)\n"),
        Opt("output_directory", 0, Kind::PATH, &P::output_directory).paragraph(
            "        --output_directory <output_directory>                          output directory\n"),
        Opt("posterior_threshold", 0, Kind::F64, &P::posterior_threshold).paragraph(
            "        --posterior_threshold <posterior_threshold>                    posterior threshold for assignment (default 0.999)\n"),
        Opt("ref", 'r', Kind::PATH, &P::ref_mtx).paragraph(
            "    -r, --ref <ref>                                                    ref.mtx matrix from vartrix\n"),
        Opt("vcf", 'v', Kind::PATH, &P::vcf).as("--vcf <vcf>").paragraph(
            "    -v, --vcf <vcf>                                                    vcf associated with alt.mtx and ref.mtx\n"),
        Opt("device", 0, Kind::USIZE, &P::device).paragraph(
            "        --device <n>                                                   run on this one GPU (not in the reference)\n"),
        Opt("devices", 0, Kind::DEVICES, std::monostate()).paragraph(
            "        --devices <a,b,...>                                            GPUs to shard the cells over, RCCL exchanges between them (not in\n"
            "                                                                       the reference; default: GPU 0; `auto`: one visible GPU per 4 GB of\n"
            "                                                                       alt.mtx text; a GPU listed twice = two logical shards on it)\n"),
        Opt("resolve_near_ties", 0, Kind::WORD, &P::resolve_near_ties).one_of("false|true", "expected true or false")
            .on_one_gpu("--resolve_near_ties true").paragraph(
            "        --resolve_near_ties <true|false>                               evaluate the cells next to the median, the quartiles and the\n"
            "                                                                       threshold with the reference's own arithmetic, so that they get\n"
            "                                                                       the reference's bits (not in the reference; default false; one GPU)\n"),
        Opt("resolve_assignments", 0, Kind::WORD, &P::resolve_assignments).one_of("false|true|all", "expected true, false or all")
            .on_one_gpu("--resolve_assignments %s").paragraph(
            "        --resolve_assignments <true|false|all>                         --resolve_near_ties, and posteriors, labels and quals of the cells\n"
            "                                                                       next to a decision edge (all: of every cell) in the reference's\n"
            "                                                                       own arithmetic: cellector_assignments.tsv then has the reference's\n"
            "                                                                       labels and quals (all: its bytes) (not in the reference; default\n"
            "                                                                       false; one GPU)\n"),
        Opt("normalization", 0, Kind::WORD, &P::zscore).one_of("per_locus|zscore", "expected per_locus or zscore").paragraph(
            "        --normalization <per_locus|zscore>                             the outlier score of a cell: its log likelihood per used locus (the\n"
            "                                                                       reference's, default) or the z-score (log likelihood - expected) /\n"
            "                                                                       sqrt(expected variance) the reference's author left commented out;\n"
            "                                                                       zscore adds a column expected_log_variance to iteration_N.tsv and\n"
            "                                                                       cannot be used with --resolve_near_ties true / --resolve_assignments\n"
            "                                                                       (not in the reference; --interquartile_range_multiple's default was\n"
            "                                                                       chosen for per_locus)\n"),
        Opt("locus_expected", 0, Kind::WORD, &P::locus_expected).one_of("false|true", "expected true or false")
            .on_one_gpu("--locus_expected true").paragraph(
            "        --locus_expected <true|false>                                  iteration_N_locus_contribution.tsv: the columns expected_loglike_minority /\n"
            "                                                                       _majority hold the expected log likelihood of the locus' entries (the\n"
            "                                                                       reference fills them with a copy of the two columns before them), and\n"
            "                                                                       four columns are appended: variance_minority, variance_majority,\n"
            "                                                                       zscore_minority, zscore_majority = (log likelihood - expected) /\n"
            "                                                                       sqrt(variance) (not in the reference; default false; one GPU)\n"),
        Opt("initial_minority", 0, Kind::PATH, &P::initial_minority).paragraph(
            "        --initial_minority <file>                                      start the loop from these cells as the excluded (minority) set\n"
            "                                                                       instead of the empty set: one barcode per line, first tab-separated\n"
            "                                                                       column (a filtered cellector_assignments.tsv works), blank lines\n"
            "                                                                       ignored (not in the reference)\n"),
        Opt("cell_detail", 0, Kind::PATH, &P::cell_detail).paragraph(
            "        --cell_detail <file>                                               write <output_directory>/cell_detail.tsv: one row per matrix entry of\n"
            "                                                                       each listed cell with its log-pmf, expected log-pmf and variance\n"
            "                                                                       under the final alpha / beta and its log-pmf under the minority,\n"
            "                                                                       majority and doublet distributions of the posterior; one barcode\n"
            "                                                                       per line, first tab-separated column, blank lines ignored (not in\n"
            "                                                                       the reference)\n"),
        Opt("cells", 0, Kind::PATH, &P::cells).on_one_gpu("--cells").paragraph(
            "        --cells <file>                                                 run on the listed cells only, as if barcodes.tsv held only these\n"
            "                                                                       lines (in its own order) and both matrices only these columns,\n"
            "                                                                       renumbered; the matrix is cut on the GPU after the load; one barcode\n"
            "                                                                       per line, first tab-separated column, blank lines ignored (not in\n"
            "                                                                       the reference; one GPU)\n"),
        Opt("downsample_rate", 0, Kind::F64, &P::downsample_rate).as("--downsample_rate <r>").within(RATE, "expected a number in [0, 1]")
            .on_one_gpu("--downsample_rate").paragraph(
            "        --downsample_rate <r>                                          remove every read with probability r in [0, 1] after the load, the\n"
            "                                                                       meaning of the combiner's flag of this name (not in the reference;\n"
            "                                                                       one GPU)\n"),
        Opt("seed", 0, Kind::USIZE, &P::seed).paragraph(
            "        --seed <n>                                                     seed of --downsample_rate's draw (default 4)\n"),
        Opt("mix_alt", 0, Kind::PATH, &P::mix_alt).on_one_gpu("--mix_alt").paragraph(
            "        --mix_alt <alt2> --mix_ref <ref2> --mix_barcodes <barcodes2>   merge a second dataset in on the GPU after the load, as the combiner\n"
            "                                                                       writes two datasets into one: its cells behind the first one's, its\n"
            "                                                                       barcodes with the last character replaced by 2; both datasets must\n"
            "                                                                       come from the same variant VCF (equal locus counts).  The three are\n"
            "                                                                       given together.  barcodes.tsv and gt.tsv (majority / minority) of\n"
            "                                                                       the mixture are written to the output directory; without -g that\n"
            "                                                                       gt.tsv is the ground truth.  --cells, --downsample_rate and --seed\n"
            "                                                                       act on the first dataset, --mix_cells and the same rate and seed on\n"
            "                                                                       the second (not in the reference; one GPU)\n"),
        Opt("mix_ref", 0, Kind::PATH, &P::mix_ref),
        Opt("mix_barcodes", 0, Kind::PATH, &P::mix_barcodes),
        Opt("mix_cells", 0, Kind::PATH, &P::mix_cells).paragraph(
            "        --mix_cells <file>                                             take only the listed cells of the second dataset (its own barcodes,\n"
            "                                                                       one per line, first tab-separated column, blank lines ignored)\n"),
        Opt("doublets", 0, Kind::PATH, &P::doublets).as("--doublets <file>").on_one_gpu("--doublets").paragraph(
            "        --doublets <file>                                              add one synthetic doublet per line of the file on the GPU, after\n"
            "                                                                       --cells, --downsample_rate and --mix_*: two barcodes per line,\n"
            "                                                                       tab-separated, blank lines ignored, named as the run's cells are\n"
            "                                                                       after those flags (as in the run's barcodes.tsv).  The new cell\n"
            "                                                                       <A>+<B> holds the sum of the two cells' counts at every locus either\n"
            "                                                                       covers and follows all other cells; a pair may be listed once.\n"
            "                                                                       barcodes.tsv and gt.tsv are written to the output directory: the\n"
            "                                                                       cells there before keep their label (-g's, else the mixture's, else\n"
            "                                                                       singlet), the new cells get doublet unless -g names them; that\n"
            "                                                                       gt.tsv is the run's ground truth (not in the reference; one GPU)\n"),
        Opt("doublet_downsample_rate", 0, Kind::F64, &P::doublet_downsample_rate).as("--doublet_downsample_rate <r>")
            .within(RATE, "expected a number in [0, 1]").requires_option("doublets").paragraph(
            "        --doublet_downsample_rate <r>                                  remove every read of a parent with probability r in [0, 1] on its\n"
            "                                                                       way into a doublet, independently per pair and parent (default 0;\n"
            "                                                                       --seed is shared)\n"),
        Opt("classes", 0, Kind::PATH, &P::classes).as("--classes <file>").paragraph(
            "        --classes <file>                                               after the ordinary run, score every cell against the genotype\n"
            "                                                                       classes of this file: barcode<TAB>label per line, at most 16\n"
            "                                                                       distinct labels (numbered by first appearance); a barcode not\n"
            "                                                                       listed is unlabelled.  Writes <output_directory>/\n"
            "                                                                       cellector_classes.tsv: barcode, input label, class_assignment\n"
            "                                                                       (the best class' label when its posterior exceeds\n"
            "                                                                       --posterior_threshold and the cell has at least\n"
            "                                                                       --min_loci_for_assignment entries, else unassigned), qual, the\n"
            "                                                                       K log-likelihoods, the K posteriors.  No other output changes\n"
            "                                                                       (not in the reference; one GPU)\n"),
        Opt("refine_classes", 0, Kind::USIZE, &P::refine_classes).as("--refine_classes <max_iter>")
            .within({0.0, 4294967295.0, false, false}, nullptr).paragraph(
            "        --refine_classes <max_iter>                                    with --classes: move every cell to its best class and score\n"
            "                                                                       again, until no cell moves or max_iter steps have run (default\n"
            "                                                                       0); one stderr line per step: cells moved, class sizes\n"),
        Opt("class_doublets", 0, Kind::WORD, &P::class_doublets).as("--class_doublets true").one_of("false|true", "expected true or false").paragraph(
            "        --class_doublets <true|false>                                  with --classes: score the doublet class of every pair of classes\n"
            "                                                                       beside them; class_assignment is doublet where the doublet\n"
            "                                                                       posterior exceeds 0.5, cellector_classes.tsv gains the columns\n"
            "                                                                       doublet_posterior and doublet_pair (<labelA>+<labelB> or na), and\n"
            "                                                                       --refine_classes holds the called doublets out of the classes'\n"
            "                                                                       tallies (its stderr line gains held=<n>) (default false)\n"),
        Opt("class_genotypes", 0, Kind::WORD, &P::class_genotypes).as("--class_genotypes true").one_of("false|true", "expected true or false")
            .requires_option("vcf").on_one_gpu("--class_genotypes true").paragraph(
            "        --class_genotypes <true|false>                                 with --classes and --vcf: writes cellector_classes.vcf, the input\n"
            "                                                                       vcf with one sample column GT:GP:AO:RO per class, called like\n"
            "                                                                       the two of cellector.vcf from the reads of the cells whose\n"
            "                                                                       class_assignment is that class (doublet and unassigned cells\n"
            "                                                                       are in none), and cellector_class_concordance.tsv: per pair of\n"
            "                                                                       classes the loci both are called at and those where the calls\n"
            "                                                                       differ (default false; one GPU)\n"),
        Opt("cluster", 0, Kind::USIZE, &P::cluster).as("--cluster <K>").within({2.0, 16.0, false, false}, "expected 2..16")
            .on_one_gpu("--cluster <K>").paragraph(
            "        --cluster <K>                                                      after the ordinary run, fit K genotype clusters (2..16) without\n"
            "                                                                       any labels: a binomial mixture by annealed soft EM over random\n"
            "                                                                       restarts (--seed is shared).  Writes <output_directory>/\n"
            "                                                                       cellector_clusters.tsv: barcode, cluster (0..K-1, unassigned for a\n"
            "                                                                       cell without an entry), the K posteriors, the K log-likelihoods.\n"
            "                                                                       Without --classes the clusters are the classes of\n"
            "                                                                       --refine_classes, --class_doublets and --class_genotypes; with\n"
            "                                                                       --classes it is a usage error.  No other output changes (not in\n"
            "                                                                       the reference; one GPU)\n"),
        Opt("cluster_restarts", 0, Kind::USIZE, &P::cluster_restarts).as("--cluster_restarts <R>").requires_option("cluster").paragraph(
            "        --cluster_restarts <R>                                             with --cluster: random restarts run side by side, K R <= 64\n"
            "                                                                       (default min(16, 64 / K))\n"),
        Opt("cluster_mask", 0, Kind::WORD, &P::cluster_mask_loop).as("--cluster_mask <all|loop>").one_of("all|loop", "expected all or loop")
            .requires_option("cluster").paragraph(
            "        --cluster_mask <all|loop>                                          with --cluster: fit on every used locus, or on the loci the\n"
            "                                                                       loop's last iteration used (default all)\n"),
        Opt("donors", 0, Kind::PATH, &P::donors).as("--donors <vcf>").requires_option("vcf").on_one_gpu("--donors <vcf>").paragraph(
            "        --donors <vcf>                                                     after the ordinary run, score every cell against the genotyped\n"
            "                                                                       donors of the pool: a VCF with one sample column per donor (at\n"
            "                                                                       most 64), matched to --vcf's records by chrom, pos, ref and alt; a\n"
            "                                                                       missing record or call counts as no call.  Writes\n"
            "                                                                       <output_directory>/cellector_donors.tsv: barcode, singlet /\n"
            "                                                                       doublet / ambiguous / unassigned, donor, second donor, best pair,\n"
            "                                                                       the three posteriors, n_loci, the donors' log-likelihoods.  With\n"
            "                                                                       --classes or --cluster also cellector_cluster_donors.tsv: class,\n"
            "                                                                       cells, donor, margin, the donors' sums.  Needs --vcf.  No other\n"
            "                                                                       output changes (not in the reference; one GPU)\n"),
        Opt("donor_error", 0, Kind::F64, &P::donor_error).as("--donor_error").within({0.0, 0.5, true, true}, "expected a number in (0, 0.5)")
            .requires_option("donors").paragraph(
            "        --donor_error <e>                                                  with --donors: allele fraction of a homozygous call (default 0.01)\n"),
        Opt("donor_ambient", 0, Kind::F64, &P::donor_ambient).as("--donor_ambient").within({0.0, 1.0, false, true}, "expected a number in [0, 1)")
            .requires_option("donors").paragraph(
            "        --donor_ambient <a>                                                with --donors: share of ambient reads (default 0.03)\n"),
        Opt("donor_doublet_rate", 0, Kind::F64, &P::donor_doublet_rate).as("--donor_doublet_rate")
            .within({0.0, 1.0, false, true}, "expected a number in [0, 1)").requires_option("donors").paragraph(
            "        --donor_doublet_rate <r>                                           with --donors: prior mass of the doublets (default 0.1)\n"),
        Opt("donor_field", 0, Kind::WORD_USAGE, &P::donor_field).as("--donor_field <GT|GP|GL|PL>").one_of("GT|GP|GL|PL", "expected GT, GP, GL or PL")
            .requires_option("donors").paragraph(
            "        --donor_field <GT|GP|GL|PL>                                        with --donors: what to read of a donor's sample (default GT, the\n"
            "                                                                       hard call).  GP: three genotype probabilities; GL: log10\n"
            "                                                                       likelihoods, 10^(GL - max GL); PL: phred-scaled ones,\n"
            "                                                                       10^(-(PL - min PL) / 10).  A cell's term is then the mixture over\n"
            "                                                                       the donor's three genotypes under those weights, and\n"
            "                                                                       cellector_donors.tsv and cellector_cluster_donors.tsv carry the\n"
            "                                                                       same columns.  A sample without a usable field falls back to its\n"
            "                                                                       GT, then to no call.  --estimate_ambient keeps scoring hard calls,\n"
            "                                                                       the most probable genotype of every row (the soft ambient profile\n"
            "                                                                       is not implemented).  With GT no output changes\n"),
        Opt("donor_panel", 0, Kind::USIZE, &P::donor_panel).as("--donor_panel <M>").within({1.0, 64.0, false, false}, "expected a number in 1..64")
            .requires_option("donors").paragraph(
            "        --donor_panel <M>                                                  with --donors: the VCF is a PANEL of 1..4096 genotyped donors\n"
            "                                                                       (hard calls: not with --donor_field GP|GL|PL).  Every cell is\n"
            "                                                                       scored against all of them and the doublets of its best donor\n"
            "                                                                       with its M best ones (1..64) in one softmax.  Writes\n"
            "                                                                       cellector_donor_panel.tsv (barcode, status, donor, second_donor,\n"
            "                                                                       best_pair, the three posteriors, n_loci and per shortlist slot\n"
            "                                                                       candidate_j, log_likelihood_j, posterior_j) and\n"
            "                                                                       cellector_donor_panel_donors.tsv (donor, singlet_cells,\n"
            "                                                                       doublet_cells, present), with --classes or --cluster also\n"
            "                                                                       cellector_cluster_panel_donors.tsv.  The donors that are present\n"
            "                                                                       then are the donors of the ordinary donor pass, as if the VCF\n"
            "                                                                       held only their columns; with none or more than 64 present\n"
            "                                                                       that pass is skipped (not in the reference)\n"),
        Opt("donor_panel_min_cells", 0, Kind::USIZE, &P::donor_panel_min_cells).as("--donor_panel_min_cells <n>")
            .within({1.0, 1e18, false, false}, "expected a number >= 1").requires_option("donor_panel").paragraph(
            "        --donor_panel_min_cells <n>                                        with --donor_panel: a donor is present with at least n cells\n"
            "                                                                       called singlets of it (default 1)\n"),
        Opt("estimate_ambient", 0, Kind::WORD, &P::estimate_ambient).as("--estimate_ambient <true|apply>")
            .one_of("false|true|apply", "expected true, apply or false").requires_option("donors").paragraph(
            "        --estimate_ambient <true|apply>                                    with --donors: measure the pool's share of ambient reads from\n"
            "                                                                       the cells the donor pass calls singlets, each under its best\n"
            "                                                                       donor (a profile likelihood over a grid that zooms in).  Writes\n"
            "                                                                       cellector_ambient.tsv (the pool and every donor: cells, rho,\n"
            "                                                                       se) and cellector_ambient_cells.tsv (barcode, donor, n_loci,\n"
            "                                                                       rho, se; NA for a cell that took no part).  true: no other\n"
            "                                                                       output changes.  apply: the donor pass runs again with the\n"
            "                                                                       pooled estimate as its ambient share and those results are\n"
            "                                                                       written; not with --donor_ambient (not in the reference)\n"),
        Opt("donor_fit", 0, Kind::WORD, &P::donor_fit).as("--donor_fit true").one_of("false|true", "expected true or false")
            .requires_option("donors").paragraph(
            "        --donor_fit <true>                                                 with --donors: how well the hypothesis the donor pass chose\n"
            "                                                                       explains every cell, z = (ll - expected) / sqrt(variance), and\n"
            "                                                                       the cells whose z lies below the singlets' lower quartile by\n"
            "                                                                       more than k interquartile ranges: cells of a donor the VCF does\n"
            "                                                                       not hold.  Writes cellector_donor_fit.tsv (barcode, status,\n"
            "                                                                       donor, second donor of a called pair, n_loci, ll, expected,\n"
            "                                                                       variance, z, unmatched) and prints one line; no other output\n"
            "                                                                       changes.  Under --donor_field GP|GL|PL it scores every row's\n"
            "                                                                       most probable genotype (not in the reference)\n"),
        Opt("donor_fit_iqr", 0, Kind::F64, &P::donor_fit_iqr).as("--donor_fit_iqr <k>").within({0.0, INFINITY, false, false}, "expected a number >= 0")
            .requires_option("donor_fit").paragraph(
            "        --donor_fit_iqr <k>                                                with --donor_fit: the multiple k (default 3)\n"),
        Opt("doublet_fraction", 0, Kind::WORD, &P::doublet_fraction).as("--doublet_fraction true").one_of("false|true", "expected true or false")
            .requires_option("donors").paragraph(
            "        --doublet_fraction <true>                                          with --donors: the share of every called doublet's reads that\n"
            "                                                                       come from its first donor, a profile likelihood over the grid\n"
            "                                                                       0, 1/16 ... 1 under (the donor pass' anchor, its best pair),\n"
            "                                                                       after the second donor pass of --estimate_ambient apply.\n"
            "                                                                       Writes cellector_doublet_fractions.tsv (barcode, donor_a,\n"
            "                                                                       donor_b, n_loci, fraction, se, ll_half, ll_max, kind: balanced,\n"
            "                                                                       toward_a, toward_b or flat; NA for a cell that is no doublet)\n"
            "                                                                       and prints one line; no other output changes.  A contaminated\n"
            "                                                                       singlet leans to one donor, a doublet of two like cells is\n"
            "                                                                       balanced.  Under --donor_field GP|GL|PL it scores every row's\n"
            "                                                                       most probable genotype (not in the reference)\n"),
        Opt("doublet_min_fraction", 0, Kind::F64, &P::doublet_min_fraction).as("--doublet_min_fraction <m>")
            .within({0.0, 0.5, false, false}, "expected a number in [0, 0.5]").requires_option("doublet_fraction").paragraph(
            "        --doublet_min_fraction <m>                                         with --doublet_fraction: a share above 1 - m leans toward_a, one\n"
            "                                                                       below m toward_b (default 0.1)\n"),
        Opt("donor_genotypes", 0, Kind::WORD, &P::donor_genotypes).as("--donor_genotypes <true|apply>")
            .one_of("false|true|apply", "expected true, apply or false").requires_option("donors").paragraph(
            "        --donor_genotypes <true|apply>                                     with --donors: the donors' genotypes from the reads of the cells\n"
            "                                                                       the donor pass calls singlets, each under its best donor, after\n"
            "                                                                       the second donor pass of --estimate_ambient apply and with the\n"
            "                                                                       ambient share in force.  The donors' own rows are the prior (GP,\n"
            "                                                                       GL, PL as read; GT as one-hot rows), floored at 0.01.  Writes\n"
            "                                                                       cellector_donor_genotypes.vcf (the records of --vcf, one\n"
            "                                                                       GT:GP:AO:RO column per donor, ./. below a posterior of 0.99)\n"
            "                                                                       and cellector_donor_genotypes.tsv (donor, cells,\n"
            "                                                                       loci_with_reads, confirmed, filled, changed, withdrawn) and\n"
            "                                                                       prints one line.  true: no other output changes.  apply: the\n"
            "                                                                       donor pass runs once more with the refined genotypes as\n"
            "                                                                       weights, and cellector_donors.tsv, --donor_fit,\n"
            "                                                                       --doublet_fraction and the class match are written from that\n"
            "                                                                       pass (not in the reference)\n"),
        Opt("matrix_pair", 0, Kind::WORD_USAGE, &P::matrix_pair).as("--matrix_pair <aligned|join|depth>")
            .one_of("aligned|join|depth", "expected aligned, join or depth").on_one_gpu("--matrix_pair %s").paragraph(
            "        --matrix_pair <aligned|join|depth>                                 how the lines of -a and -r belong together.  aligned (default):\n"
            "                                                                       line i of -r belongs to line i of -a, the reference's reading;\n"
            "                                                                       the indices of -r are never looked at.  join: the two files are\n"
            "                                                                       joined by (locus, cell) on the GPU; either may lack the other's\n"
            "                                                                       keys (dropped zero lines) and be in any order, a missing count\n"
            "                                                                       is 0.  depth: the same join, -r holding the total depth alt + ref\n"
            "                                                                       (an AD / DP pair); a key whose depth is below its alt count is an\n"
            "                                                                       error.  A key listed twice in one file is an error in both.  The\n"
            "                                                                       --mix_alt / --mix_ref pair is read the same way.  One stderr line\n"
            "                                                                       counts the keys; no output changes (not in the reference; one GPU)\n"),
        Opt("write_matrices", 0, Kind::WORD_USAGE, &P::write_matrices).as("--write_matrices <aligned|sparse|depth>")
            .one_of("off|aligned|sparse|depth", "expected aligned, sparse or depth").on_one_gpu("--write_matrices %s").paragraph(
            "        --write_matrices <aligned|sparse|depth>                            write the matrix the run works on, after --matrix_pair, --cells,\n"
            "                                                                       --downsample_rate, --mix_* and --doublets and before the locus\n"
            "                                                                       filter, into the output directory as text formatted on the GPU,\n"
            "                                                                       tab-separated with the combiner's header.  aligned: alt.mtx and\n"
            "                                                                       ref.mtx, one line per entry, zeros explicit (the combiner's files;\n"
            "                                                                       read back by default).  sparse: the same two names with the zero\n"
            "                                                                       lines dropped (read back with --matrix_pair join).  depth: ad.mtx\n"
            "                                                                       and dp.mtx, alt and alt + ref (read back with --matrix_pair depth).\n"
            "                                                                       barcodes.tsv of the run's cells is written beside them where\n"
            "                                                                       --mix_* or --doublets do not write it already.  An input of the\n"
            "                                                                       run under one of these names in the output directory is refused.\n"
            "                                                                       One stderr line gives the counts; no other output changes (not in\n"
            "                                                                       the reference; one GPU)\n"),
        Opt("write_matrices_gz", 0, Kind::WORD, &P::write_matrices_gz).as("--write_matrices_gz true").one_of("false|true", "expected true or false")
            .requires_option("write_matrices").paragraph(
            "        --write_matrices_gz <true>                                         with --write_matrices: the same two files as alt.mtx.gz and\n"
            "                                                                       ref.mtx.gz (ad.mtx.gz and dp.mtx.gz), block-compressed gzip (BGZF,\n"
            "                                                                       what bgzip writes) made on the GPU: zcat, gzip -t and -a / -r of\n"
            "                                                                       this program read them.  The stderr line gains the compressed\n"
            "                                                                       sizes (not in the reference)\n"),
        Opt("gz_device", 0, Kind::WORD, &P::gz_device).as("--gz_device true").one_of("false|true", "expected true or false").paragraph(
            "        --gz_device <true|false>                                           a block-compressed .gz (BGZF: bgzip's, --write_matrices_gz's)\n"
            "                                                                       given as -a / -r or --mix_alt / --mix_ref goes to the GPU\n"
            "                                                                       compressed and is inflated there, under every --matrix_pair; a\n"
            "                                                                       plain file or a plain gzip is read as ever, and so is every file\n"
            "                                                                       of a run on several GPUs.  No output changes (not in the\n"
            "                                                                       reference; default false)\n"),
    };
    return table;
}
inline const Opt *find_option(const std::string &name)
{
    for (const Opt &o : options())
        if (name == o.name) return &o;
    return nullptr;
}

// --help: the rows' paragraphs in table order under the fixed head
inline std::string usage()
{
    std::string u =
        "cellector 1.0.0\nHaynes Heaton <whheaton@gmail.com>\ngenotype outlier detection for scRNAseq\n\n"
        "USAGE:\n    cellector [OPTIONS] --alt <alt> --barcodes <barcodes> --output_directory <output_directory> --ref <ref>\n\n"
        "OPTIONS:\n";
    for (const Opt &o : options())
        if (o.help) u += o.help;
    return u;
}

// ---- the value parse: one routine per kind ------------------------------------------------------------------------
inline uint64_t parse_usize(const std::string &name, const std::string &s)
{
    uint64_t v = 0;
    auto r = std::from_chars(s.data(), s.data() + s.size(), v);
    if (s.empty() || r.ec != std::errc() || r.ptr != s.data() + s.size())
        die(EXIT_PANIC, "invalid value '" + s + "' for --" + name + ": expected an unsigned integer");
    return v;
}
inline double parse_f64(const std::string &name, const std::string &s)
{
    char *end = nullptr;
    double v = strtod(s.c_str(), &end);
    if (s.empty() || end != s.c_str() + s.size()) die(EXIT_PANIC, "invalid value '" + s + "' for --" + name + ": expected a number");
    return v;
}
[[noreturn]] inline void die_invalid_value(const Opt &o, const std::string &text)
{
    die(1, "error: Invalid value '" + text + "' for '" + o.shown + "'" + (o.expected ? std::string(": ") + o.expected : ""));
}
inline void check_range(const Opt &o, double v, const std::string &text)
{
    if (!o.range) return;
    const Range &r = *o.range;
    if (!((r.lo_open ? v > r.lo : v >= r.lo) && (r.hi_open ? v < r.hi : v <= r.hi))) die_invalid_value(o, text);  // (a NaN is outside)
}
// a WORD's place in the row's list
inline uint64_t parse_word(const Opt &o, const std::string &text)
{
    const std::vector<std::string> words = split(o.words, '|');
    const size_t at = std::find(words.begin(), words.end(), text) - words.begin();
    if (at < words.size()) return at;
    if (o.kind == Kind::WORD_USAGE) die_invalid_value(o, text);
    die(EXIT_PANIC, "invalid value '" + text + "' for --" + o.name + ": " + o.expected);
}
inline void store(Params &p, const Opt &o, const std::string &text)
{
    uint64_t u = 0;
    double d = 0.0;
    switch (o.kind) {
    case Kind::PATH: break;
    case Kind::USIZE: u = parse_usize(o.name, text); check_range(o, (double)u, text); break;
    case Kind::F64: d = parse_f64(o.name, text); check_range(o, d, text); break;
    case Kind::WORD:
    case Kind::WORD_USAGE: u = parse_word(o, text); break;
    case Kind::DEVICES:
        if (text == "auto") p.devices_auto = true;
        else
            for (const std::string &t : split(text, ',')) p.devices.push_back((int)parse_usize("devices", t));
        break;
    }
    std::visit([&](auto member) {
        using M = decltype(member);
        if constexpr (std::is_same_v<M, std::string Params::*> || std::is_same_v<M, std::optional<std::string> Params::*>) p.*member = text;
        else if constexpr (std::is_same_v<M, uint64_t Params::*>) p.*member = u;
        else if constexpr (std::is_same_v<M, int Params::*>) p.*member = (int)u;
        else if constexpr (std::is_same_v<M, bool Params::*>) p.*member = u != 0;
        else if constexpr (!std::is_same_v<M, std::monostate>) p.*member = d;
    }, o.field);
}

inline Params load_params(int argc, char **argv)
{
    std::map<std::string, std::string> got;
    for (int i = 1; i < argc; i++) {
        std::string a = argv[i], name, value;
        bool have_value = false;
        if (a == "-h" || a == "--help") { fputs(usage().c_str(), stdout); exit(0); }
        if (a == "-V" || a == "--version") { puts("cellector 1.0.0"); exit(0); }
        if (a.rfind("--", 0) == 0) {
            size_t eq = a.find('=');
            name = a.substr(2, eq == std::string::npos ? std::string::npos : eq - 2);
            if (eq != std::string::npos) { value = a.substr(eq + 1); have_value = true; }
        } else if (a.size() >= 2 && a[0] == '-') {
            for (const Opt &o : options())
                if (o.short_name == a[1]) name = o.name;
            if (a.size() > 2) { value = a.substr(a[2] == '=' ? 3 : 2); have_value = true; }
        }
        if (name.empty() || !find_option(name))
            die(1, "error: Found argument '" + a + "' which wasn't expected, or isn't valid in this context\n\n" + usage());
        if (!have_value) {
            if (i + 1 >= argc) die(1, "error: The argument '--" + name + " <" + name + ">' requires a value but none was supplied");
            value = argv[++i];
        }
        if (got.count(name)) die(1, "error: The argument '--" + name + " <" + name + ">' was provided more than once");
        got[name] = value;
    }
    for (const char *req : {"alt", "barcodes", "output_directory", "ref"})
        if (!got.count(req)) die(1, std::string("error: The following required arguments were not provided:\n    --") + req + " <" + req + ">\n\n" + usage());
    // an option is in force when it was given and, a <true|false> one, not with false: what "requires" and the one-GPU rule ask
    auto in_force = [&](const Opt &o) {
        const auto at = got.find(o.name);
        return at != got.end() && !((o.kind == Kind::WORD || o.kind == Kind::WORD_USAGE) && at->second == "false");
    };
    Params p;
    for (const Opt &o : options()) {
        if (!got.count(o.name)) continue;
        store(p, o, got[o.name]);
        if (o.needs && in_force(o) && !in_force(*find_option(o.needs)))
            die(1, std::string("error: The argument '") + o.shown + "' requires '" + find_option(o.needs)->shown + "'");
    }

    // relations between two options
    if (got.count("device") && got.count("devices")) die(1, "error: The argument '--device <n>' cannot be used with '--devices <a,b,...>'");
    if (p.zscore && p.resolve_near_ties)
        die(1, "error: The argument '--normalization zscore' cannot be used with '--resolve_near_ties true': the reference has no "
               "arithmetic of that score to resolve to");
    if (p.zscore && p.resolve_assignments)
        die(1, "error: The argument '--normalization zscore' cannot be used with '--resolve_assignments " + got["resolve_assignments"] +
                   "': the reference has no arithmetic of that score to resolve to");
    if (p.write_matrices_gz && !p.write_matrices)
        die(1, "error: The argument '--write_matrices_gz true' requires '--write_matrices <aligned|sparse|depth>'");
    if (p.cluster && p.classes) die(1, "error: The argument '--cluster <K>' cannot be used with '--classes <file>'");
    if (got.count("cluster_restarts") && (p.cluster_restarts < 1 || p.cluster_restarts * p.cluster > 64))
        die(1, "error: Invalid value '" + got["cluster_restarts"] + "' for '--cluster_restarts <R>': expected 1..64 / K");
    // (--cluster's clusters serve as the classes of these three)
    for (const char *flag : {"class_doublets", "class_genotypes", "refine_classes"})
        if (in_force(*find_option(flag)) && !p.classes && !p.cluster)
            die(1, std::string("error: The argument '") + find_option(flag)->shown + "' requires '--classes <file>'");
    if (p.donor_panel && p.donor_field != "GT")
        die(1, "error: The argument '--donor_panel <M>' cannot be used with '--donor_field " + p.donor_field + "': a panel is scored from hard calls");
    if (p.estimate_ambient == 2 && got.count("donor_ambient"))
        die(1, "error: The argument '--estimate_ambient apply' cannot be used with '--donor_ambient <a>'");
    if (p.mix_alt || p.mix_ref || p.mix_barcodes || p.mix_cells)
        for (const char *flag : {"mix_alt", "mix_ref", "mix_barcodes"})
            if (!got.count(flag))
                die(1, std::string("error: The arguments '--mix_alt', '--mix_ref' and '--mix_barcodes' are given together: '--") + flag +
                           " <file>' was not provided");

    if (!p.one_gpu())
        for (const Opt &o : options())
            if (o.one_gpu && in_force(o) && !(o.kind == Kind::WORD_USAGE && got[o.name] == split(o.words, '|')[0])) {  // (its default word asks for nothing)
                std::string quoted = o.one_gpu;
                if (const size_t at = quoted.find("%s"); at != std::string::npos) quoted.replace(at, 2, got[o.name]);
                die(1, "error: The argument '" + quoted + "' works on one GPU and cannot be used with '--devices <a,b,...>'");
            }
    return p;
}
