// cellector — host binary of the MI355X build: same command line (cellector/src/params.yml), same input files
// and the same output files as the reference's Rust binary (main.rs), with the scoring path running in
// libcellector_hip.so through the C ABI of include/cellector_ffi.h.  The reference host is Rust; this image has no
// Rust toolchain, so the host above the C ABI is C++ (INTEGRATION.md shows the equivalent Rust binding).
//
// Host-side pieces restated here (cited per function): load_params (main.rs:629-677), create_output_dir /
// load_barcodes / load_ground_truth / load_vcf_data (load_data.rs:37-107), the driver loop cellector()
// (main.rs:36-50), the writers output_iteration_tsv (main.rs:349-366), locus_filter_and_output_locus_data
// (main.rs:422-498), output_final_assignments + pretty_print (main.rs:133-226), output_final_vcf (main.rs:52-131).
#include <sys/stat.h>
#include <zlib.h>

#include <algorithm>
#include <charconv>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <unistd.h>
#include <cstdlib>
#include <cstring>
#include <map>
#include <numeric>
#include <optional>
#include <chrono>
#include <string>
#include <string_view>
#include <thread>
#include <unordered_map>
#include <vector>

#include "../include/cellector_ffi.h"
#include "donor_vcf_host.h"
#include "genotype_host.h"

namespace {

constexpr int EXIT_PANIC = 101;  // what a Rust panic gives the caller (cellector_pipeline.py checks != 0 only)
[[noreturn]] void die(int code, const std::string &msg)
{
    fprintf(stderr, "%s\n", msg.c_str());
    exit(code);
}

// ---- Rust `{}` formatting of f64: shortest round-trip digits, never scientific --------
std::string fmt(double v)
{
    if (std::isnan(v)) return "NaN";
    if (std::isinf(v)) return v > 0 ? "inf" : "-inf";
    char buf[400];
    auto r = std::to_chars(buf, buf + sizeof buf, v, std::chars_format::fixed);
    return std::string(buf, r.ptr);
}
std::string fmt(uint64_t v) { return std::to_string(v); }
// the same, appended to a row under construction
void put(std::string &o, double v)
{
    if (std::isnan(v)) { o += "NaN"; return; }
    if (std::isinf(v)) { o += v > 0 ? "inf" : "-inf"; return; }
    char buf[400];
    auto r = std::to_chars(buf, buf + sizeof buf, v, std::chars_format::fixed);
    o.append(buf, r.ptr);
}
void put(std::string &o, uint64_t v)
{
    char buf[24];
    auto r = std::to_chars(buf, buf + sizeof buf, v);
    o.append(buf, r.ptr);
}
// Formats rows [0, n) with row(i, out) on several host threads (contiguous ranges) and writes them in order: at 1M cells
// the reference-shaped fprintf loops were a visible part of the run once the scoring itself takes milliseconds.
template <class F>
void write_rows(FILE *f, uint64_t n, F row)
{
    unsigned nt = std::thread::hardware_concurrency();
    if (nt > 16) nt = 16;
    if (nt < 1 || n < 20000) nt = 1;
    std::vector<std::string> buf(nt);
    auto work = [&](unsigned t) {
        const uint64_t b = n * t / nt, e = n * (t + 1) / nt;
        buf[t].reserve((size_t)(e - b) * 96);
        for (uint64_t i = b; i < e; i++) row(i, buf[t]);
    };
    std::vector<std::thread> th;
    for (unsigned t = 1; t < nt; t++) th.emplace_back(work, t);
    work(0);
    for (auto &x : th) x.join();
    for (unsigned t = 0; t < nt; t++) fwrite(buf[t].data(), 1, buf[t].size(), f);
}

// ---- reader (load_data.rs:240-251): ".gz" by extension, multi-member ------------------------------------------
struct Lines {
    gzFile gz = nullptr;
    std::string cur;
    explicit Lines(const std::string &path)
    {
        gz = gzopen(path.c_str(), "rb");  // transparent for plain files
        if (!gz) die(EXIT_PANIC, "couldn't open file " + path);
        gzbuffer(gz, 1 << 20);
    }
    ~Lines() { if (gz) gzclose(gz); }
    bool next(std::string &out)  // BufRead::lines(): strips "\n" and a preceding "\r"
    {
        out.clear();
        char buf[1 << 16];
        bool any = false;
        while (gzgets(gz, buf, sizeof buf)) {
            any = true;
            size_t n = strlen(buf);
            if (n && buf[n - 1] == '\n') {
                out.append(buf, n - 1);
                if (!out.empty() && out.back() == '\r') out.pop_back();
                return true;
            }
            out.append(buf, n);
        }
        return any;
    }
};

// the bytes of a (possibly gzipped) text file
std::string read_whole(const std::string &path)
{
    gzFile gz = gzopen(path.c_str(), "rb");  // transparent for plain files
    if (!gz) die(EXIT_PANIC, "couldn't open file " + path);
    gzbuffer(gz, 1 << 20);
    std::string out;
    std::vector<char> buf(4 << 20);
    for (;;) {
        const int n = gzread(gz, buf.data(), (unsigned)buf.size());
        if (n <= 0) break;
        out.append(buf.data(), (size_t)n);
    }
    gzclose(gz);
    return out;
}
// BufRead::lines() over a buffer: "\n" ends a line, a "\r" in front of it is dropped, a last line needs no terminator
std::vector<std::string_view> split_lines(const std::string &text)
{
    std::vector<std::string_view> out;
    out.reserve(text.size() / 16 + 1);
    size_t b = 0;
    while (b < text.size()) {
        size_t e = text.find('\n', b);
        const size_t next = e == std::string::npos ? text.size() : e + 1;
        if (e == std::string::npos) e = text.size();
        size_t len = e - b;
        if (len && e < text.size() && text[e] == '\n' && text[e - 1] == '\r') len--;  // (only a terminated line loses its "\r")
        out.emplace_back(text.data() + b, len);
        b = next;
    }
    return out;
}

std::vector<std::string> split(const std::string &s, char sep)
{
    std::vector<std::string> out;
    size_t b = 0;
    for (;;) {
        size_t e = s.find(sep, b);
        if (e == std::string::npos) { out.push_back(s.substr(b)); return out; }
        out.push_back(s.substr(b, e - b));
        b = e + 1;
    }
}

// ---- load_params (main.rs:629-677, params.yml) -----------------------------------------------------------------
struct Params {
    std::string ref_mtx, alt_mtx, barcodes, output_directory;
    std::optional<std::string> ground_truth, vcf;
    uint64_t min_alt = 4, min_ref = 4, min_alleles_posterior = 5, min_loci_used = 30;
    double posterior_threshold = 0.999, interquartile_range_multiple = 5.0;
    std::optional<double> expected_percent_minority;  // parsed, never used (quirk Q2)
    int device = -1;                                   // extension: ONE GPU to run on
    std::vector<int> devices;                          // extension: the GPUs to shard the cells over (default: GPU 0)
    bool devices_auto = false;                         // --devices auto: as many visible GPUs as the input can feed
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
    // extension: the pool's ambient fraction measured from the donor pass' singlets (cellector_estimate_ambient)
    std::string donor_field = "GT";                    // GT: hard calls; GP, GL, PL: the donors' genotype weights (cellector_donor_posteriors_gp)
    int estimate_ambient = 0;                          // 0 = off, 1 = true: report it, 2 = apply: and score the donors again with it
    // extension: the fit of every cell's called hypothesis, and the cells no genotyped donor explains (cellector_donor_fit)
    bool donor_fit = false;
    std::optional<double> donor_fit_iqr;               // the multiple of the iqr below the lower quartile (default: the library's, 3)
};

const char *USAGE =
    "cellector 1.0.0\nHaynes Heaton <whheaton@gmail.com>\ngenotype outlier detection for scRNAseq\n\n"
    "USAGE:\n    cellector [OPTIONS] --alt <alt> --barcodes <barcodes> --output_directory <output_directory> --ref <ref>\n\n"
    "OPTIONS:\n"
    "    -a, --alt <alt>                                                    alt.mtx matrix from vartrix\n"
    "    -b, --barcodes <barcodes>                                          cell barcodes\n"
    "        --expected_percent_minority <expected_percent_minority>        percent of cells expected to come from the minority genotype\n"
    "    -g, --ground_truth <ground_truth>                                  cell hashing assignments or other ground truth\n"
    "        --interquartile_range_multiple <interquartile_range_multiple>  IQR multiples below the 25th percentile for the outlier threshold\n"
    "        --min_alleles_posterior <min_alleles_posterior>                minimum alleles per distribution for the posterior calculation\n"
    "        --min_alt <min_alt>                                            minimum number of cells containing the alt allele (default 4)\n"
    "        --min_loci_for_assignment <min_loci_for_assignment>            minimum loci to assign a cell (default 30)\n"
    "        --min_ref <min_ref>                                            minimum number of cells containing the ref allele (default 4)\n"
    "        --output_directory <output_directory>                          output directory\n"
    "        --posterior_threshold <posterior_threshold>                    posterior threshold for assignment (default 0.999)\n"
    "    -r, --ref <ref>                                                    ref.mtx matrix from vartrix\n"
    "    -v, --vcf <vcf>                                                    vcf associated with alt.mtx and ref.mtx\n"
    "        --device <n>                                                   run on this one GPU (not in the reference)\n"
    "        --devices <a,b,...>                                            GPUs to shard the cells over, RCCL exchanges between them (not in\n"
    "                                                                       the reference; default: GPU 0; `auto`: one visible GPU per 4 GB of\n"
    "                                                                       alt.mtx text; a GPU listed twice = two logical shards on it)\n"
    "        --resolve_near_ties <true|false>                               evaluate the cells next to the median, the quartiles and the\n"
    "                                                                       threshold with the reference's own arithmetic, so that they get\n"
    "                                                                       the reference's bits (not in the reference; default false; one GPU)\n"
    "        --resolve_assignments <true|false|all>                         --resolve_near_ties, and posteriors, labels and quals of the cells\n"
    "                                                                       next to a decision edge (all: of every cell) in the reference's\n"
    "                                                                       own arithmetic: cellector_assignments.tsv then has the reference's\n"
    "                                                                       labels and quals (all: its bytes) (not in the reference; default\n"
    "                                                                       false; one GPU)\n"
    "        --normalization <per_locus|zscore>                             the outlier score of a cell: its log likelihood per used locus (the\n"
    "                                                                       reference's, default) or the z-score (log likelihood - expected) /\n"
    "                                                                       sqrt(expected variance) the reference's author left commented out;\n"
    "                                                                       zscore adds a column expected_log_variance to iteration_N.tsv and\n"
    "                                                                       cannot be used with --resolve_near_ties true / --resolve_assignments\n"
    "                                                                       (not in the reference; --interquartile_range_multiple's default was\n"
    "                                                                       chosen for per_locus)\n"
    "        --locus_expected <true|false>                                  iteration_N_locus_contribution.tsv: the columns expected_loglike_minority /\n"
    "                                                                       _majority hold the expected log likelihood of the locus' entries (the\n"
    "                                                                       reference fills them with a copy of the two columns before them), and\n"
    "                                                                       four columns are appended: variance_minority, variance_majority,\n"
    "                                                                       zscore_minority, zscore_majority = (log likelihood - expected) /\n"
    "                                                                       sqrt(variance) (not in the reference; default false; one GPU)\n"
    "        --initial_minority <file>                                      start the loop from these cells as the excluded (minority) set\n"
    "                                                                       instead of the empty set: one barcode per line, first tab-separated\n"
    "                                                                       column (a filtered cellector_assignments.tsv works), blank lines\n"
    "                                                                       ignored (not in the reference)\n"
    "        --cell_detail <file>                                               write <output_directory>/cell_detail.tsv: one row per matrix entry of\n"
    "                                                                       each listed cell with its log-pmf, expected log-pmf and variance\n"
    "                                                                       under the final alpha / beta and its log-pmf under the minority,\n"
    "                                                                       majority and doublet distributions of the posterior; one barcode\n"
    "                                                                       per line, first tab-separated column, blank lines ignored (not in\n"
    "                                                                       the reference)\n"
    "        --cells <file>                                                 run on the listed cells only, as if barcodes.tsv held only these\n"
    "                                                                       lines (in its own order) and both matrices only these columns,\n"
    "                                                                       renumbered; the matrix is cut on the GPU after the load; one barcode\n"
    "                                                                       per line, first tab-separated column, blank lines ignored (not in\n"
    "                                                                       the reference; one GPU)\n"
    "        --downsample_rate <r>                                          remove every read with probability r in [0, 1] after the load, the\n"
    "                                                                       meaning of the combiner's flag of this name (not in the reference;\n"
    "                                                                       one GPU)\n"
    "        --seed <n>                                                     seed of --downsample_rate's draw (default 4)\n"
    "        --mix_alt <alt2> --mix_ref <ref2> --mix_barcodes <barcodes2>   merge a second dataset in on the GPU after the load, as the combiner\n"
    "                                                                       writes two datasets into one: its cells behind the first one's, its\n"
    "                                                                       barcodes with the last character replaced by 2; both datasets must\n"
    "                                                                       come from the same variant VCF (equal locus counts).  The three are\n"
    "                                                                       given together.  barcodes.tsv and gt.tsv (majority / minority) of\n"
    "                                                                       the mixture are written to the output directory; without -g that\n"
    "                                                                       gt.tsv is the ground truth.  --cells, --downsample_rate and --seed\n"
    "                                                                       act on the first dataset, --mix_cells and the same rate and seed on\n"
    "                                                                       the second (not in the reference; one GPU)\n"
    "        --mix_cells <file>                                             take only the listed cells of the second dataset (its own barcodes,\n"
    "                                                                       one per line, first tab-separated column, blank lines ignored)\n"
    "        --doublets <file>                                              add one synthetic doublet per line of the file on the GPU, after\n"
    "                                                                       --cells, --downsample_rate and --mix_*: two barcodes per line,\n"
    "                                                                       tab-separated, blank lines ignored, named as the run's cells are\n"
    "                                                                       after those flags (as in the run's barcodes.tsv).  The new cell\n"
    "                                                                       <A>+<B> holds the sum of the two cells' counts at every locus either\n"
    "                                                                       covers and follows all other cells; a pair may be listed once.\n"
    "                                                                       barcodes.tsv and gt.tsv are written to the output directory: the\n"
    "                                                                       cells there before keep their label (-g's, else the mixture's, else\n"
    "                                                                       singlet), the new cells get doublet unless -g names them; that\n"
    "                                                                       gt.tsv is the run's ground truth (not in the reference; one GPU)\n"
    "        --doublet_downsample_rate <r>                                  remove every read of a parent with probability r in [0, 1] on its\n"
    "                                                                       way into a doublet, independently per pair and parent (default 0;\n"
    "                                                                       --seed is shared)\n"
    "        --classes <file>                                               after the ordinary run, score every cell against the genotype\n"
    "                                                                       classes of this file: barcode<TAB>label per line, at most 16\n"
    "                                                                       distinct labels (numbered by first appearance); a barcode not\n"
    "                                                                       listed is unlabelled.  Writes <output_directory>/\n"
    "                                                                       cellector_classes.tsv: barcode, input label, class_assignment\n"
    "                                                                       (the best class' label when its posterior exceeds\n"
    "                                                                       --posterior_threshold and the cell has at least\n"
    "                                                                       --min_loci_for_assignment entries, else unassigned), qual, the\n"
    "                                                                       K log-likelihoods, the K posteriors.  No other output changes\n"
    "                                                                       (not in the reference; one GPU)\n"
    "        --refine_classes <max_iter>                                    with --classes: move every cell to its best class and score\n"
    "                                                                       again, until no cell moves or max_iter steps have run (default\n"
    "                                                                       0); one stderr line per step: cells moved, class sizes\n"
    "        --class_doublets <true|false>                                  with --classes: score the doublet class of every pair of classes\n"
    "                                                                       beside them; class_assignment is doublet where the doublet\n"
    "                                                                       posterior exceeds 0.5, cellector_classes.tsv gains the columns\n"
    "                                                                       doublet_posterior and doublet_pair (<labelA>+<labelB> or na), and\n"
    "                                                                       --refine_classes holds the called doublets out of the classes'\n"
    "                                                                       tallies (its stderr line gains held=<n>) (default false)\n"
    "        --class_genotypes <true|false>                                 with --classes and --vcf: writes cellector_classes.vcf, the input\n"
    "                                                                       vcf with one sample column GT:GP:AO:RO per class, called like\n"
    "                                                                       the two of cellector.vcf from the reads of the cells whose\n"
    "                                                                       class_assignment is that class (doublet and unassigned cells\n"
    "                                                                       are in none), and cellector_class_concordance.tsv: per pair of\n"
    "                                                                       classes the loci both are called at and those where the calls\n"
    "                                                                       differ (default false; one GPU)\n"
    "        --cluster <K>                                                      after the ordinary run, fit K genotype clusters (2..16) without\n"
    "                                                                       any labels: a binomial mixture by annealed soft EM over random\n"
    "                                                                       restarts (--seed is shared).  Writes <output_directory>/\n"
    "                                                                       cellector_clusters.tsv: barcode, cluster (0..K-1, unassigned for a\n"
    "                                                                       cell without an entry), the K posteriors, the K log-likelihoods.\n"
    "                                                                       Without --classes the clusters are the classes of\n"
    "                                                                       --refine_classes, --class_doublets and --class_genotypes; with\n"
    "                                                                       --classes it is a usage error.  No other output changes (not in\n"
    "                                                                       the reference; one GPU)\n"
    "        --cluster_restarts <R>                                             with --cluster: random restarts run side by side, K R <= 64\n"
    "                                                                       (default min(16, 64 / K))\n"
    "        --cluster_mask <all|loop>                                          with --cluster: fit on every used locus, or on the loci the\n"
    "                                                                       loop's last iteration used (default all)\n"
    "        --donors <vcf>                                                     after the ordinary run, score every cell against the genotyped\n"
    "                                                                       donors of the pool: a VCF with one sample column per donor (at\n"
    "                                                                       most 64), matched to --vcf's records by chrom, pos, ref and alt; a\n"
    "                                                                       missing record or call counts as no call.  Writes\n"
    "                                                                       <output_directory>/cellector_donors.tsv: barcode, singlet /\n"
    "                                                                       doublet / ambiguous / unassigned, donor, second donor, best pair,\n"
    "                                                                       the three posteriors, n_loci, the donors' log-likelihoods.  With\n"
    "                                                                       --classes or --cluster also cellector_cluster_donors.tsv: class,\n"
    "                                                                       cells, donor, margin, the donors' sums.  Needs --vcf.  No other\n"
    "                                                                       output changes (not in the reference; one GPU)\n"
    "        --donor_error <e>                                                  with --donors: allele fraction of a homozygous call (default 0.01)\n"
    "        --donor_ambient <a>                                                with --donors: share of ambient reads (default 0.03)\n"
    "        --donor_doublet_rate <r>                                           with --donors: prior mass of the doublets (default 0.1)\n"
    "        --donor_field <GT|GP|GL|PL>                                        with --donors: what to read of a donor's sample (default GT, the\n"
    "                                                                       hard call).  GP: three genotype probabilities; GL: log10\n"
    "                                                                       likelihoods, 10^(GL - max GL); PL: phred-scaled ones,\n"
    "                                                                       10^(-(PL - min PL) / 10).  A cell's term is then the mixture over\n"
    "                                                                       the donor's three genotypes under those weights, and\n"
    "                                                                       cellector_donors.tsv and cellector_cluster_donors.tsv carry the\n"
    "                                                                       same columns.  A sample without a usable field falls back to its\n"
    "                                                                       GT, then to no call.  --estimate_ambient keeps scoring hard calls,\n"
    "                                                                       the most probable genotype of every row (the soft ambient profile\n"
    "                                                                       is not implemented).  With GT no output changes\n"
    "        --estimate_ambient <true|apply>                                    with --donors: measure the pool's share of ambient reads from\n"
    "                                                                       the cells the donor pass calls singlets, each under its best\n"
    "                                                                       donor (a profile likelihood over a grid that zooms in).  Writes\n"
    "                                                                       cellector_ambient.tsv (the pool and every donor: cells, rho,\n"
    "                                                                       se) and cellector_ambient_cells.tsv (barcode, donor, n_loci,\n"
    "                                                                       rho, se; NA for a cell that took no part).  true: no other\n"
    "                                                                       output changes.  apply: the donor pass runs again with the\n"
    "                                                                       pooled estimate as its ambient share and those results are\n"
    "                                                                       written; not with --donor_ambient (not in the reference)\n"
    "        --donor_fit <true>                                                 with --donors: how well the hypothesis the donor pass chose\n"
    "                                                                       explains every cell, z = (ll - expected) / sqrt(variance), and\n"
    "                                                                       the cells whose z lies below the singlets' lower quartile by\n"
    "                                                                       more than k interquartile ranges: cells of a donor the VCF does\n"
    "                                                                       not hold.  Writes cellector_donor_fit.tsv (barcode, status,\n"
    "                                                                       donor, second donor of a called pair, n_loci, ll, expected,\n"
    "                                                                       variance, z, unmatched) and prints one line; no other output\n"
    "                                                                       changes.  Under --donor_field GP|GL|PL it scores every row's\n"
    "                                                                       most probable genotype (not in the reference)\n"
    "        --donor_fit_iqr <k>                                                with --donor_fit: the multiple k (default 3)\n";

uint64_t parse_usize(const std::string &name, const std::string &s)
{
    uint64_t v = 0;
    auto r = std::from_chars(s.data(), s.data() + s.size(), v);
    if (s.empty() || r.ec != std::errc() || r.ptr != s.data() + s.size())
        die(EXIT_PANIC, "invalid value '" + s + "' for --" + name + ": expected an unsigned integer");
    return v;
}
double parse_f64(const std::string &name, const std::string &s)
{
    char *end = nullptr;
    double v = strtod(s.c_str(), &end);
    if (s.empty() || end != s.c_str() + s.size()) die(EXIT_PANIC, "invalid value '" + s + "' for --" + name + ": expected a number");
    return v;
}

Params load_params(int argc, char **argv)
{
    static const std::map<std::string, std::string> shorts = {{"-r", "ref"}, {"-a", "alt"}, {"-b", "barcodes"},
                                                              {"-g", "ground_truth"}, {"-v", "vcf"}};
    static const char *known[] = {"output_directory", "ref", "alt", "barcodes", "min_alt", "min_ref", "ground_truth",
                                  "vcf", "posterior_threshold", "interquartile_range_multiple", "min_alleles_posterior",
                                  "expected_percent_minority", "min_loci_for_assignment", "device", "devices",
                                  "resolve_near_ties", "resolve_assignments", "initial_minority", "cell_detail", "normalization",
                                  "locus_expected", "cells", "downsample_rate", "seed", "mix_alt", "mix_ref", "mix_barcodes",
                                  "mix_cells", "doublets", "doublet_downsample_rate", "classes", "refine_classes",
                                  "class_doublets", "class_genotypes", "cluster", "cluster_restarts", "cluster_mask", "donors",
                                  "donor_error", "donor_ambient", "donor_doublet_rate", "donor_field", "estimate_ambient", "donor_fit",
                                  "donor_fit_iqr"};
    std::map<std::string, std::string> got;
    for (int i = 1; i < argc; i++) {
        std::string a = argv[i], name, value;
        bool have_value = false;
        if (a == "-h" || a == "--help") { fputs(USAGE, stdout); exit(0); }
        if (a == "-V" || a == "--version") { puts("cellector 1.0.0"); exit(0); }
        if (a.rfind("--", 0) == 0) {
            size_t eq = a.find('=');
            name = a.substr(2, eq == std::string::npos ? std::string::npos : eq - 2);
            if (eq != std::string::npos) { value = a.substr(eq + 1); have_value = true; }
        } else if (shorts.count(a.substr(0, 2))) {
            name = shorts.at(a.substr(0, 2));
            if (a.size() > 2) { value = a.substr(a[2] == '=' ? 3 : 2); have_value = true; }
        } else {
            die(1, "error: Found argument '" + a + "' which wasn't expected, or isn't valid in this context\n\n" + USAGE);
        }
        if (std::find_if(std::begin(known), std::end(known), [&](const char *k) { return name == k; }) == std::end(known))
            die(1, "error: Found argument '" + a + "' which wasn't expected, or isn't valid in this context\n\n" + USAGE);
        if (!have_value) {
            if (i + 1 >= argc) die(1, "error: The argument '--" + name + " <" + name + ">' requires a value but none was supplied");
            value = argv[++i];
        }
        if (got.count(name)) die(1, "error: The argument '--" + name + " <" + name + ">' was provided more than once");
        got[name] = value;
    }
    for (const char *req : {"alt", "barcodes", "output_directory", "ref"})
        if (!got.count(req)) die(1, std::string("error: The following required arguments were not provided:\n    --") + req + " <" + req + ">\n\n" + USAGE);
    Params p;
    p.ref_mtx = got["ref"]; p.alt_mtx = got["alt"]; p.barcodes = got["barcodes"]; p.output_directory = got["output_directory"];
    if (got.count("ground_truth")) p.ground_truth = got["ground_truth"];
    if (got.count("vcf")) p.vcf = got["vcf"];
    if (got.count("min_alt")) p.min_alt = parse_usize("min_alt", got["min_alt"]);
    if (got.count("min_ref")) p.min_ref = parse_usize("min_ref", got["min_ref"]);
    if (got.count("posterior_threshold")) p.posterior_threshold = parse_f64("posterior_threshold", got["posterior_threshold"]);
    if (got.count("interquartile_range_multiple"))
        p.interquartile_range_multiple = parse_f64("interquartile_range_multiple", got["interquartile_range_multiple"]);
    if (got.count("min_alleles_posterior")) p.min_alleles_posterior = parse_usize("min_alleles_posterior", got["min_alleles_posterior"]);
    if (got.count("expected_percent_minority")) p.expected_percent_minority = parse_f64("expected_percent_minority", got["expected_percent_minority"]);
    if (got.count("min_loci_for_assignment")) p.min_loci_used = parse_usize("min_loci_for_assignment", got["min_loci_for_assignment"]);
    if (got.count("device")) p.device = (int)parse_usize("device", got["device"]);
    if (got.count("devices")) {
        if (got["devices"] == "auto") p.devices_auto = true;
        else
            for (const std::string &t : split(got["devices"], ',')) p.devices.push_back((int)parse_usize("devices", t));
    }
    if (got.count("device") && got.count("devices")) die(1, "error: The argument '--device <n>' cannot be used with '--devices <a,b,...>'");
    if (got.count("resolve_near_ties")) {
        const std::string &v = got["resolve_near_ties"];
        if (v != "true" && v != "false") die(EXIT_PANIC, "invalid value '" + v + "' for --resolve_near_ties: expected true or false");
        p.resolve_near_ties = v == "true";
    }
    if (got.count("resolve_assignments")) {
        const std::string &v = got["resolve_assignments"];
        if (v != "true" && v != "false" && v != "all")
            die(EXIT_PANIC, "invalid value '" + v + "' for --resolve_assignments: expected true, false or all");
        p.resolve_assignments = v == "true" ? 1 : (v == "all" ? 2 : 0);
    }
    if (got.count("normalization")) {
        const std::string &v = got["normalization"];
        if (v != "per_locus" && v != "zscore") die(EXIT_PANIC, "invalid value '" + v + "' for --normalization: expected per_locus or zscore");
        p.zscore = v == "zscore";
    }
    if (p.zscore && p.resolve_near_ties)
        die(1, "error: The argument '--normalization zscore' cannot be used with '--resolve_near_ties true': the reference has no "
               "arithmetic of that score to resolve to");
    if (p.zscore && p.resolve_assignments)
        die(1, "error: The argument '--normalization zscore' cannot be used with '--resolve_assignments " + got["resolve_assignments"] +
                   "': the reference has no arithmetic of that score to resolve to");
    if (got.count("locus_expected")) {
        const std::string &v = got["locus_expected"];
        if (v != "true" && v != "false") die(EXIT_PANIC, "invalid value '" + v + "' for --locus_expected: expected true or false");
        p.locus_expected = v == "true";
    }
    if (got.count("initial_minority")) p.initial_minority = got["initial_minority"];
    if (got.count("cell_detail")) p.cell_detail = got["cell_detail"];
    if (got.count("cells")) p.cells = got["cells"];
    if (got.count("downsample_rate")) {
        const double r = parse_f64("downsample_rate", got["downsample_rate"]);
        if (!(r >= 0.0 && r <= 1.0)) die(1, "error: Invalid value '" + got["downsample_rate"] + "' for '--downsample_rate <r>': expected a number in [0, 1]");
        p.downsample_rate = r;
    }
    if (got.count("seed")) p.seed = parse_usize("seed", got["seed"]);
    if (got.count("classes")) p.classes = got["classes"];
    if (got.count("cluster")) {
        p.cluster = parse_usize("cluster", got["cluster"]);
        if (p.cluster < 2 || p.cluster > 16) die(1, "error: Invalid value '" + got["cluster"] + "' for '--cluster <K>': expected 2..16");
        if (p.classes) die(1, "error: The argument '--cluster <K>' cannot be used with '--classes <file>'");
        if (p.devices_auto || p.devices.size() > 1)
            die(1, "error: The argument '--cluster <K>' works on one GPU and cannot be used with '--devices <a,b,...>'");
    }
    if (got.count("cluster_restarts")) {
        p.cluster_restarts = parse_usize("cluster_restarts", got["cluster_restarts"]);
        if (!p.cluster) die(1, "error: The argument '--cluster_restarts <R>' requires '--cluster <K>'");
        if (p.cluster_restarts < 1 || p.cluster_restarts * p.cluster > 64)
            die(1, "error: Invalid value '" + got["cluster_restarts"] + "' for '--cluster_restarts <R>': expected 1..64 / K");
    }
    if (got.count("cluster_mask")) {
        const std::string &v = got["cluster_mask"];
        if (v != "all" && v != "loop") die(EXIT_PANIC, "invalid value '" + v + "' for --cluster_mask: expected all or loop");
        if (!p.cluster) die(1, "error: The argument '--cluster_mask <all|loop>' requires '--cluster <K>'");
        p.cluster_mask_loop = v == "loop";
    }
    if (got.count("class_doublets")) {
        const std::string &v = got["class_doublets"];
        if (v != "true" && v != "false") die(EXIT_PANIC, "invalid value '" + v + "' for --class_doublets: expected true or false");
        p.class_doublets = v == "true";
        if (p.class_doublets && !p.classes && !p.cluster) die(1, "error: The argument '--class_doublets true' requires '--classes <file>'");
    }
    if (got.count("class_genotypes")) {
        const std::string &v = got["class_genotypes"];
        if (v != "true" && v != "false") die(EXIT_PANIC, "invalid value '" + v + "' for --class_genotypes: expected true or false");
        p.class_genotypes = v == "true";
        if (p.class_genotypes && !p.classes && !p.cluster) die(1, "error: The argument '--class_genotypes true' requires '--classes <file>'");
        if (p.class_genotypes && !p.vcf) die(1, "error: The argument '--class_genotypes true' requires '--vcf <vcf>'");
    }
    if (got.count("refine_classes")) {
        p.refine_classes = parse_usize("refine_classes", got["refine_classes"]);
        if (!p.classes && !p.cluster) die(1, "error: The argument '--refine_classes <max_iter>' requires '--classes <file>'");
        if (p.refine_classes > 0xffffffffull) die(1, "error: Invalid value '" + got["refine_classes"] + "' for '--refine_classes <max_iter>'");
    }
    if (got.count("donors")) {
        p.donors = got["donors"];
        if (!p.vcf) die(1, "error: The argument '--donors <vcf>' requires '--vcf <vcf>'");
        if (p.devices_auto || p.devices.size() > 1)
            die(1, "error: The argument '--donors <vcf>' works on one GPU and cannot be used with '--devices <a,b,...>'");
    }
    for (const char *flag : {"donor_error", "donor_ambient", "donor_doublet_rate"})
        if (got.count(flag)) {
            if (!p.donors) die(1, std::string("error: The argument '--") + flag + "' requires '--donors <vcf>'");
            const double v = parse_f64(flag, got[flag]);
            const std::string f = flag;
            const bool ok = f == "donor_error" ? v > 0.0 && v < 0.5 : v >= 0.0 && v < 1.0;
            if (!ok) die(1, "error: Invalid value '" + got[flag] + "' for '--" + f + "': expected a number in " + (f == "donor_error" ? "(0, 0.5)" : "[0, 1)"));
            (f == "donor_error" ? p.donor_error : f == "donor_ambient" ? p.donor_ambient : p.donor_doublet_rate) = v;
        }
    if (got.count("donor_field")) {
        if (!p.donors) die(1, "error: The argument '--donor_field <GT|GP|GL|PL>' requires '--donors <vcf>'");
        p.donor_field = got["donor_field"];
        if (p.donor_field != "GT" && p.donor_field != "GP" && p.donor_field != "GL" && p.donor_field != "PL")
            die(1, "error: Invalid value '" + p.donor_field + "' for '--donor_field <GT|GP|GL|PL>': expected GT, GP, GL or PL");
    }
    if (got.count("estimate_ambient")) {
        const std::string &v = got["estimate_ambient"];
        if (v != "true" && v != "apply" && v != "false")
            die(EXIT_PANIC, "invalid value '" + v + "' for --estimate_ambient: expected true, apply or false");
        p.estimate_ambient = v == "true" ? 1 : v == "apply" ? 2 : 0;
        if (p.estimate_ambient && !p.donors) die(1, "error: The argument '--estimate_ambient <true|apply>' requires '--donors <vcf>'");
        if (p.estimate_ambient == 2 && got.count("donor_ambient"))
            die(1, "error: The argument '--estimate_ambient apply' cannot be used with '--donor_ambient <a>'");
    }
    if (got.count("donor_fit")) {
        const std::string &v = got["donor_fit"];
        if (v != "true" && v != "false") die(EXIT_PANIC, "invalid value '" + v + "' for --donor_fit: expected true or false");
        p.donor_fit = v == "true";
        if (p.donor_fit && !p.donors) die(1, "error: The argument '--donor_fit true' requires '--donors <vcf>'");
    }
    if (got.count("donor_fit_iqr")) {
        if (!p.donor_fit) die(1, "error: The argument '--donor_fit_iqr <k>' requires '--donor_fit true'");
        const double v = parse_f64("donor_fit_iqr", got["donor_fit_iqr"]);
        if (!(v >= 0.0)) die(1, "error: Invalid value '" + got["donor_fit_iqr"] + "' for '--donor_fit_iqr <k>': expected a number >= 0");
        p.donor_fit_iqr = v;
    }
    if (got.count("mix_alt")) p.mix_alt = got["mix_alt"];
    if (got.count("mix_ref")) p.mix_ref = got["mix_ref"];
    if (got.count("mix_barcodes")) p.mix_barcodes = got["mix_barcodes"];
    if (got.count("mix_cells")) p.mix_cells = got["mix_cells"];
    if (p.mix_alt || p.mix_ref || p.mix_barcodes || p.mix_cells)
        for (const char *flag : {"mix_alt", "mix_ref", "mix_barcodes"})
            if (!got.count(flag))
                die(1, std::string("error: The arguments '--mix_alt', '--mix_ref' and '--mix_barcodes' are given together: '--") + flag +
                           " <file>' was not provided");
    if (got.count("doublets")) p.doublets = got["doublets"];
    if (got.count("doublet_downsample_rate")) {
        const double r = parse_f64("doublet_downsample_rate", got["doublet_downsample_rate"]);
        if (!(r >= 0.0 && r <= 1.0))
            die(1, "error: Invalid value '" + got["doublet_downsample_rate"] + "' for '--doublet_downsample_rate <r>': expected a number in [0, 1]");
        p.doublet_downsample_rate = r;
        if (!p.doublets) die(1, "error: The argument '--doublet_downsample_rate <r>' requires '--doublets <file>'");
    }
    for (const char *flag : {"cells", "downsample_rate", "mix_alt", "doublets"})
        if (got.count(flag) && (p.devices_auto || p.devices.size() > 1))
            die(1, std::string("error: The argument '--") + flag + "' works on one GPU and cannot be used with '--devices <a,b,...>'");
    if (p.resolve_assignments && (p.devices_auto || p.devices.size() > 1))
        die(1, "error: The argument '--resolve_assignments " + got["resolve_assignments"] +
                   "' works on one GPU and cannot be used with '--devices <a,b,...>'");
    if (p.locus_expected && (p.devices_auto || p.devices.size() > 1))
        die(1, "error: The argument '--locus_expected true' works on one GPU and cannot be used with '--devices <a,b,...>'");
    if (p.class_genotypes && (p.devices_auto || p.devices.size() > 1))
        die(1, "error: The argument '--class_genotypes true' works on one GPU and cannot be used with '--devices <a,b,...>'");
    if (p.resolve_near_ties && (p.devices_auto || p.devices.size() > 1))
        die(1, "error: The argument '--resolve_near_ties true' works on one GPU and cannot be used with '--devices <a,b,...>'");
    return p;
}

// statrs Data::median on a copy (main.rs:442-443); NaN for empty data
double median_of(std::vector<double> v)
{
    if (v.empty()) return NAN;
    std::sort(v.begin(), v.end());
    const size_t k = v.size() / 2;
    return v.size() % 2 ? v[k] : (v[k - 1] + v[k]) / 2.0;
}

// the lines of the input vcf for the two VCF writers (main.rs:64-77): rec_of = META for a "##" line, CHROM for the "#CHROM" line,
// else the record's index, which is its locus; more records than loci is the reference's index panic
struct VcfLines {
    static constexpr uint64_t META = ~0ull, CHROM = ~0ull - 1;
    std::vector<std::string> lines;
    std::vector<uint64_t> rec_of;
};
VcfLines read_vcf_lines(const std::string &path, uint64_t total_loci)
{
    VcfLines v;
    Lines in(path);
    std::string line;
    uint64_t rec = 0;
    while (in.next(line)) {
        uint64_t kind = VcfLines::META;
        if (line.rfind("##", 0) == 0) kind = VcfLines::META;
        else if (line.rfind("#CHROM", 0) == 0) kind = VcfLines::CHROM;
        else {
            if (rec >= total_loci) die(EXIT_PANIC, "index out of bounds: vcf has more records than the matrix has loci");
            kind = rec++;
        }
        v.lines.push_back(line);
        v.rec_of.push_back(kind);
    }
    return v;
}

struct Ctx {
    cellector_ctx *c = nullptr;
    void ck(cellector_status s, const char *what)
    {
        if (s != CELLECTOR_OK) die(EXIT_PANIC, std::string(what) + ": " + (c ? cellector_last_error(c) : "no context"));
    }
};

FILE *create(const std::string &path)
{
    FILE *f = fopen(path.c_str(), "w");
    if (!f) die(EXIT_PANIC, "Unable to create file " + path);
    static std::vector<char> *bufs = new std::vector<char>[64];
    static int nb = 0;
    if (nb < 64) { bufs[nb].resize(1 << 20); setvbuf(f, bufs[nb].data(), _IOFBF, bufs[nb].size()); nb++; }
    return f;
}

struct VcfLocus { std::string chrom, pos; };

}  // namespace

int main(int argc, char **argv)
{
    const Params params = load_params(argc, argv);
    // create_output_dir (load_data.rs:66-71): non-recursive mkdir, failure ignored (quirk Q13)
    (void)mkdir(params.output_directory.c_str(), 0777);

    // load_barcodes (load_data.rs:73-83): the lines of the file; barcode -> cell index for the ground truth, a later
    // duplicate overwriting an earlier one (HashMap::insert).  The file is read whole and the table is a flat open-addressing
    // one over views into it — a std::unordered_map<std::string, size_t> of a million barcodes was 0.3-0.6 s of node
    // allocations.
    std::string barcode_text = read_whole(params.barcodes);
    std::vector<std::string_view> barcodes = split_lines(barcode_text);
    std::vector<uint32_t> bc_slot;  // line index + 1 of the LAST line with that barcode, 0 = empty
    size_t n_distinct = 0;
    auto index_barcodes = [&]() {
        n_distinct = 0;
        size_t cap = 16;
        while (cap < 2 * barcodes.size() + 2) cap <<= 1;
        bc_slot.assign(cap, 0u);
        if (barcodes.size() >= 0xffffffffull) die(EXIT_PANIC, "too many barcodes");
        for (size_t i = 0; i < barcodes.size(); i++) {
            size_t h = std::hash<std::string_view>{}(barcodes[i]) & (cap - 1);
            for (;; h = (h + 1) & (cap - 1)) {
                if (!bc_slot[h]) { bc_slot[h] = (uint32_t)i + 1; n_distinct++; break; }
                if (barcodes[bc_slot[h] - 1] == barcodes[i]) { bc_slot[h] = (uint32_t)i + 1; break; }
            }
        }
    };
    index_barcodes();
    auto barcode_to_cell = [&](std::string_view key) -> size_t {  // SIZE_MAX: not a barcode
        const size_t cap = bc_slot.size();
        for (size_t h = std::hash<std::string_view>{}(key) & (cap - 1);; h = (h + 1) & (cap - 1)) {
            if (!bc_slot[h]) return SIZE_MAX;
            if (barcodes[bc_slot[h] - 1] == key) return bc_slot[h] - 1;
        }
    };
    // --cells: from here on the barcodes file IS its listed lines, in its own order: the ground truth, the barcode lists of the
    // other flags and every output see only them, exactly as on a filtered barcodes.tsv.  The matrix follows after the load
    // (cellector_restage); all_barcodes / all_slot keep the whole file to name a barcode that --cells dropped.
    std::vector<std::string_view> all_barcodes;
    std::vector<uint32_t> all_slot, kept_lines;  // kept_lines: the line index of every kept barcode, ascending
    if (params.cells) {
        all_barcodes = barcodes;
        std::vector<uint8_t> listed(barcodes.size(), 0);
        Lines in(*params.cells);
        std::string line;
        for (size_t line_no = 1; in.next(line); line_no++) {
            const std::string bc = line.substr(0, line.find('\t'));
            if (bc.empty()) continue;
            const size_t cell = barcode_to_cell(bc);
            if (cell == SIZE_MAX)
                die(1, "error: --cells " + *params.cells + " line " + std::to_string(line_no) + ": barcode '" + bc +
                           "' is not in the barcodes file " + params.barcodes);
            listed[cell] = 1;
        }
        for (size_t i = 0; i < listed.size(); i++)
            if (listed[i]) kept_lines.push_back((uint32_t)i);
        if (kept_lines.empty()) die(1, "error: --cells " + *params.cells + " lists no barcode");
        all_slot = bc_slot;
        barcodes.clear();
        for (const uint32_t i : kept_lines) barcodes.push_back(all_barcodes[i]);
        index_barcodes();
    }
    // --mix_*: the second dataset's barcodes (those --mix_cells lists, in their file's order) follow the first one's, the last
    // character replaced by 2 (combiner/src/main.rs:174-184); from here on the barcodes file IS that list, as the combiner
    // writes it into its output's barcodes.tsv
    const size_t n_first = barcodes.size();
    std::string mix_text;
    std::vector<uint8_t> mix_keep;        // [lines of --mix_barcodes] with --mix_cells
    std::vector<std::string> mix_names;   // the renamed barcodes of the cells taken
    size_t mix_lines = 0;
    if (params.mix()) {
        mix_text = read_whole(*params.mix_barcodes);
        const std::vector<std::string_view> theirs = split_lines(mix_text);
        mix_lines = theirs.size();
        if (params.mix_cells) {
            std::map<std::string_view, size_t> line_of;  // (a later duplicate overwrites an earlier one, as load_barcodes)
            for (size_t i = 0; i < theirs.size(); i++) line_of[theirs[i]] = i;
            mix_keep.assign(theirs.size(), 0);
            Lines in(*params.mix_cells);
            std::string line;
            for (size_t line_no = 1; in.next(line); line_no++) {
                const std::string bc = line.substr(0, line.find('\t'));
                if (bc.empty()) continue;
                const auto at = line_of.find(std::string_view(bc));
                if (at == line_of.end())
                    die(1, "error: --mix_cells " + *params.mix_cells + " line " + std::to_string(line_no) + ": barcode '" + bc +
                               "' is not in the barcodes file " + *params.mix_barcodes);
                mix_keep[at->second] = 1;
            }
            if (std::find(mix_keep.begin(), mix_keep.end(), 1) == mix_keep.end())
                die(1, "error: --mix_cells " + *params.mix_cells + " lists no barcode");
        }
        for (size_t i = 0; i < theirs.size(); i++) {
            if (params.mix_cells && !mix_keep[i]) continue;
            std::string bc(theirs[i]);
            if (!bc.empty()) bc.pop_back();
            bc += '2';
            mix_names.push_back(std::move(bc));
        }
        for (const std::string &bc : mix_names) barcodes.push_back(bc);  // (mix_names is complete: the views stay valid)
        index_barcodes();
    }
    // --doublets: the pairs, by the names the cells carry now; the new cells <A>+<B> follow all others, and from here on the
    // barcodes file IS that list.  The matrix follows after the load (cellector_add_doublets)
    const size_t n_before_doublets = barcodes.size();
    std::vector<uint32_t> dbl_a, dbl_b;
    std::vector<std::string> dbl_names;
    if (params.doublets) {
        Lines in(*params.doublets);
        std::string line;
        std::map<std::string, size_t> seen;  // name -> line
        for (size_t line_no = 1; in.next(line); line_no++) {
            if (line.empty()) continue;
            const std::string where = "error: --doublets " + *params.doublets + " line " + std::to_string(line_no) + ": ";
            auto cols = split(line, '\t');
            if (cols.size() != 2 || cols[0].empty() || cols[1].empty())
                die(1, where + "two tab-separated barcodes expected, got '" + line + "'");
            size_t cell[2];
            for (int k = 0; k < 2; k++) {
                cell[k] = barcode_to_cell(cols[k]);
                if (cell[k] == SIZE_MAX)
                    die(1, where + "barcode '" + cols[k] + "' is not among the run's cells (the barcodes file " + params.barcodes +
                               (params.cells ? " after --cells" : "") + (params.mix() ? ", then --mix_barcodes" : "") + ")");
            }
            if (cell[0] == cell[1]) die(1, where + "barcode '" + cols[0] + "' is paired with itself");
            std::string name = cols[0] + "+" + cols[1];
            const auto [at, fresh] = seen.emplace(name, line_no);
            if (!fresh)
                die(1, where + "the pair is line " + std::to_string(at->second) + " already: the cell '" + name + "' would exist twice");
            if (barcode_to_cell(name) != SIZE_MAX) die(1, where + "the run has a cell named '" + name + "' already");
            dbl_a.push_back((uint32_t)cell[0]);
            dbl_b.push_back((uint32_t)cell[1]);
            dbl_names.push_back(std::move(name));
        }
        if (dbl_names.empty()) die(1, "error: --doublets " + *params.doublets + " lists no pair");
        for (const std::string &bc : dbl_names) barcodes.push_back(bc);  // (dbl_names is complete: the views stay valid)
        index_barcodes();
    }
    auto dropped_by_cells = [&](std::string_view key) {  // a barcode of the whole file that --cells left out
        if (all_slot.empty()) return false;
        const size_t cap = all_slot.size();
        for (size_t h = std::hash<std::string_view>{}(key) & (cap - 1);; h = (h + 1) & (cap - 1)) {
            if (!all_slot[h]) return false;
            if (all_barcodes[all_slot[h] - 1] == key) return true;
        }
    };
    // load_ground_truth (load_data.rs:85-107): one label per DISTINCT barcode (the vector has the map's length)
    std::vector<std::string> ground_truth(n_distinct, "na");
    if (params.ground_truth) {
        Lines in(*params.ground_truth);
        std::string line;
        while (in.next(line)) {
            auto cols = split(line, '\t');
            if (cols.size() != 2) die(EXIT_PANIC, "Invalid line format: " + line + "\nThe correct format is: barcode\tassignment");
            const size_t cell = barcode_to_cell(cols[0]);
            if (cell != SIZE_MAX && cell < ground_truth.size()) ground_truth[cell] = cols[1];
        }
    }
    // the combiner's barcodes.tsv and gt.tsv of the mixture (main.rs:155-186); without -g the run's ground truth.  With --doublets
    // the cells there before keep the label in force (-g's, else the mixture's, else singlet) and the new ones are doublet
    if (params.mix() || params.doublets) {
        std::string bc_out, gt_out;
        for (size_t i = 0; i < barcodes.size(); i++) {
            std::string label = i >= n_before_doublets ? "doublet" : params.mix() ? (i < n_first ? "majority" : "minority") : "singlet";
            const size_t cell = barcode_to_cell(barcodes[i]);
            if (params.doublets && params.ground_truth && cell < ground_truth.size()) {  // -g's label; a new cell it does not name stays doublet
                if (i < n_before_doublets || ground_truth[cell] != "na") label = ground_truth[cell];
            }
            bc_out += barcodes[i]; bc_out += '\n';
            gt_out += barcodes[i]; gt_out += '\t'; gt_out += label; gt_out += '\n';
            if ((!params.ground_truth || i >= n_before_doublets) && cell < ground_truth.size()) ground_truth[cell] = label;
        }
        // an input of this run under one of the two names in the output directory would be lost: refuse before either is written
        for (const char *name : {"barcodes.tsv", "gt.tsv"}) {
            const std::string path = params.output_directory + "/" + name;
            struct stat mine, theirs;
            if (stat(path.c_str(), &mine) != 0) continue;
            for (const auto &[flag, in] : std::vector<std::pair<const char *, std::optional<std::string>>>{
                     {"--barcodes", params.barcodes}, {"--ground_truth", params.ground_truth}, {"--mix_barcodes", params.mix_barcodes},
                     {"--mix_cells", params.mix_cells}, {"--cells", params.cells}, {"--doublets", params.doublets},
                     {"--initial_minority", params.initial_minority},
                     {"--cell_detail", params.cell_detail}})
                if (in && stat(in->c_str(), &theirs) == 0 && mine.st_dev == theirs.st_dev && mine.st_ino == theirs.st_ino)
                    die(1, std::string(params.mix() ? "error: the mixture's " : "error: the run's ") + name + " would overwrite the " + flag + " file " + *in +
                               ": choose another --output_directory");
        }
        auto write_text = [&](const char *name, const std::string &text) {
            const std::string path = params.output_directory + "/" + name;
            FILE *f = fopen(path.c_str(), "w");
            if (!f) die(EXIT_PANIC, "Unable to create file " + path);
            fwrite(text.data(), 1, text.size(), f);
            fclose(f);
        };
        write_text("barcodes.tsv", bc_out);
        write_text("gt.tsv", gt_out);
    }

    // a barcode list of an extension flag: one per line, first tab-separated column, blank lines ignored; file order, repeats kept
    auto read_barcode_list = [&](const char *flag, const std::string &path) {
        std::vector<uint32_t> cells;
        Lines in(path);
        std::string line;
        for (size_t line_no = 1; in.next(line); line_no++) {
            const std::string bc = line.substr(0, line.find('\t'));
            if (bc.empty()) continue;
            const size_t cell = barcode_to_cell(bc);
            if (cell == SIZE_MAX && dropped_by_cells(bc))
                die(1, std::string("error: --") + flag + " " + path + " line " + std::to_string(line_no) + ": barcode '" + bc +
                           "' is not among the cells --cells " + *params.cells + " keeps");
            if (cell == SIZE_MAX)
                die(1, std::string("error: --") + flag + " " + path + " line " + std::to_string(line_no) + ": barcode '" + bc +
                           "' is not in the barcodes file " + params.barcodes);
            cells.push_back((uint32_t)cell);
        }
        return cells;
    };
    // --initial_minority: the cells the loop starts from as excluded_cells (main.rs:37 has `HashSet::new()`)
    std::vector<uint32_t> initial_minority;
    if (params.initial_minority) initial_minority = read_barcode_list("initial_minority", *params.initial_minority);
    // --cell_detail: the cells whose per-locus records are written after the posterior phase
    std::vector<uint32_t> detail_cells;
    if (params.cell_detail) detail_cells = read_barcode_list("cell_detail", *params.cell_detail);

    // --classes: barcode<TAB>label, parsed like load_ground_truth (load_data.rs:85-107): a line without exactly two columns is an
    // error, a barcode the run does not have is ignored, a later line of a barcode replaces an earlier one.  Labels are numbered by
    // first appearance; a cell no line names is unlabelled (255)
    std::vector<uint8_t> class_label;
    std::vector<std::string> class_names;
    if (params.classes) {
        class_label.assign(n_distinct, 255);
        Lines in(*params.classes);
        std::string line;
        while (in.next(line)) {
            auto cols = split(line, '\t');
            if (cols.size() != 2) die(EXIT_PANIC, "Invalid line format: " + line + "\nThe correct format is: barcode\tlabel");
            size_t k = std::find(class_names.begin(), class_names.end(), cols[1]) - class_names.begin();
            if (k == class_names.size()) {
                if (k == 16) die(1, "error: --classes " + *params.classes + ": more than 16 distinct labels ('" + cols[1] + "' is the 17th)");
                class_names.push_back(cols[1]);
            }
            const size_t cell = barcode_to_cell(cols[0]);
            if (cell != SIZE_MAX && cell < class_label.size()) class_label[cell] = (uint8_t)k;
        }
        if (class_names.empty()) die(1, "error: --classes " + *params.classes + ": no label");
    }

    // CELLECTOR_TIMING=1: phase wall times on stderr (not part of the reference's output)
    const bool timing = getenv("CELLECTOR_TIMING") != nullptr;
    auto t_prev = std::chrono::steady_clock::now();
    auto lap = [&](const char *what) {
        const auto now = std::chrono::steady_clock::now();
        if (timing) fprintf(stderr, "[timing] %-24s %8.3f s\n", what, std::chrono::duration<double>(now - t_prev).count());
        t_prev = now;
    };
    // load_cell_data (load_data.rs:134-181) on the device
    // Which GPUs: --device n / --devices a,b,... as given; neither (cellector_pipeline.py:223-226 passes neither flag): GPU 0 —
    // the multi-GPU path over RCCL is opt-in until it has run on a multi-GPU node (README).  --devices auto: all visible GPUs
    // when the input is large enough to feed them (one GPU per 4 GB of alt.mtx text, i.e. >= 1.3e8 entries each: below that
    // the per-iteration exchanges and the communicator set-up cost more than the extra GPUs save); should the multi-device
    // ctx fail to come up there, the run falls back to GPU 0 with a note on stderr.
    Ctx g;
    std::vector<int> devices = params.devices;
    if (devices.empty() && params.device >= 0) devices.push_back(params.device);
    if (devices.empty() && !params.devices_auto) devices.push_back(0);
    if (devices.empty()) {
        int visible = 0;
        (void)cellector_device_count(&visible);
        struct stat sb;
        const uint64_t alt_bytes = stat(params.alt_mtx.c_str(), &sb) == 0 ? (uint64_t)sb.st_size : 0;
        const bool gz = params.alt_mtx.size() > 3 && params.alt_mtx.compare(params.alt_mtx.size() - 3, 3, ".gz") == 0;
        const uint64_t text_bytes = alt_bytes * (gz ? 4 : 1);  // (text is ~4x the .gz)
        const uint64_t want = text_bytes < (4ull << 30) ? 1 : (text_bytes + (4ull << 30) - 1) / (4ull << 30);  // (BASELINE cfg5: 30.7 GB -> 8)
        if (const char *e = getenv("CELLECTOR_DEVICES_AUTO_MAX")) visible = std::min(visible, atoi(e));
        const int n = (int)std::max<uint64_t>(1, std::min<uint64_t>(want, (uint64_t)std::min(visible, 16)));
        for (int i = 0; i < n; i++) devices.push_back(i);
    }
    cellector_status cst = cellector_create_multi(&g.c, devices.data(), (int)devices.size());
    if (cst != CELLECTOR_OK && params.devices_auto && devices.size() > 1) {
        fprintf(stderr, "cellector: the %zu-GPU context did not come up (status %d); running on GPU 0\n", devices.size(), (int)cst);
        devices.assign(1, 0);
        cst = cellector_create_multi(&g.c, devices.data(), 1);
    }
    if (cst != CELLECTOR_OK)
        die(EXIT_PANIC, "cellector: no usable MI355X device (asked for " + std::to_string(devices.size()) + ", first: " +
                            std::to_string(devices[0]) + "; there is no CPU fallback)");
    if (const char *e = getenv("CELLECTOR_ENGINE")) g.ck(cellector_set_option(g.c, "engine", atoi(e)), "engine");
    if (const char *e = getenv("CELLECTOR_BANK_ORDER")) g.ck(cellector_set_option(g.c, "bank_order", atoi(e)), "bank_order");
    g.ck(cellector_set_option(g.c, "keep_coo", params.vcf ? 1 : 0), "option");
    if (params.resolve_near_ties) g.ck(cellector_set_option(g.c, "resolve_ties", 1), "resolve_near_ties");
    if (params.resolve_assignments) {
        g.ck(cellector_set_option(g.c, "resolve_ties", params.resolve_assignments), "resolve_assignments");
        g.ck(cellector_set_option(g.c, "resolve_posteriors", params.resolve_assignments), "resolve_assignments");
    }
    if (params.zscore) g.ck(cellector_set_option(g.c, "normalization", 1), "normalization");
    if (params.locus_expected) g.ck(cellector_set_option(g.c, "locus_moments", 1), "locus_expected");
    lap("barcodes + device init");
    if (!params.restage() && !params.mix() && !params.doublets) {
        g.ck(cellector_load_mtx(g.c, params.alt_mtx.c_str(), params.ref_mtx.c_str(), params.min_alt, params.min_ref), "load_cell_data");
    } else {  // --cells / --downsample_rate: the staged matrix is cut and thinned on the device before the locus filter sees it
        g.ck(cellector_ingest_mtx(g.c, params.alt_mtx.c_str(), params.ref_mtx.c_str()), "load_cell_data");
        cellector_dims_t staged;
        g.ck(cellector_dims(g.c, &staged), "dims");
        std::vector<uint8_t> keep;
        if (params.cells) {
            keep.assign(staged.total_cells, 0);
            for (const uint32_t i : kept_lines) {
                if (i >= staged.total_cells)
                    die(1, "error: --cells: barcode '" + std::string(all_barcodes[i]) + "' is line " + std::to_string(i + 1) +
                               " of the barcodes file but the matrix has " + std::to_string(staged.total_cells) + " cells");
                keep[i] = 1;
            }
        }
        g.ck(cellector_restage(g.c, params.cells ? keep.data() : nullptr, params.downsample_rate.value_or(0.0), params.seed), "restage");
        if (params.cells) {  // the barcodes above were filtered by the same rule the library renumbers by: cellector_cell_origin says so
            std::vector<uint32_t> origin(kept_lines.size());
            g.ck(cellector_cell_origin(g.c, origin.data()), "cell_origin");
            if (origin != kept_lines) die(EXIT_PANIC, "--cells: the restaged cells are not the listed barcodes in file order");
        }
        if (params.mix()) {  // the second dataset: staged in a ctx of its own on the same GPU, merged in, released
            Ctx second;
            if (cellector_create(&second.c, devices[0]) != CELLECTOR_OK) die(EXIT_PANIC, "cellector: no second context on the device");
            second.ck(cellector_ingest_mtx(second.c, params.mix_alt->c_str(), params.mix_ref->c_str()), "load_cell_data (--mix_alt / --mix_ref)");
            cellector_dims_t ours, theirs;
            g.ck(cellector_dims(g.c, &ours), "dims");
            second.ck(cellector_dims(second.c, &theirs), "dims");
            if (ours.total_loci != theirs.total_loci)
                die(1, "error: --mix_alt " + *params.mix_alt + " has " + std::to_string(theirs.total_loci) + " loci, --alt " + params.alt_mtx +
                           " has " + std::to_string(ours.total_loci) + " loci: both datasets must come from the same variant VCF");
            if (mix_lines < theirs.total_cells)
                die(EXIT_PANIC, "index out of bounds: the barcodes file " + *params.mix_barcodes + " has " + std::to_string(mix_lines) +
                                    " lines but the matrix has " + std::to_string(theirs.total_cells) + " cells");
            std::vector<uint8_t> take;
            if (params.mix_cells) {
                for (size_t i = theirs.total_cells; i < mix_keep.size(); i++)
                    if (mix_keep[i])
                        die(1, "error: --mix_cells: a listed barcode is line " + std::to_string(i + 1) + " of " + *params.mix_barcodes +
                                   " but the matrix has " + std::to_string(theirs.total_cells) + " cells");
                take.assign(mix_keep.begin(), mix_keep.begin() + (ptrdiff_t)theirs.total_cells);
            } else if (mix_lines != theirs.total_cells) {
                die(EXIT_PANIC, "the barcodes file " + *params.mix_barcodes + " has " + std::to_string(mix_lines) + " lines but the matrix has " +
                                    std::to_string(theirs.total_cells) + " cells");
            }
            g.ck(cellector_combine(g.c, second.c, params.mix_cells ? take.data() : nullptr, nullptr, ours.total_loci,
                                   params.downsample_rate.value_or(0.0), params.seed), "combine");
            cellector_destroy(second.c);
        }
        if (params.doublets) {  // last: the pairs name the cells as they are now
            cellector_dims_t now;
            g.ck(cellector_dims(g.c, &now), "dims");
            for (size_t j = 0; j < dbl_a.size(); j++)
                for (const uint32_t cell : {dbl_a[j], dbl_b[j]})
                    if (cell >= now.total_cells)
                        die(1, "error: --doublets: barcode '" + std::string(barcodes[cell]) + "' is line " + std::to_string(cell + 1) +
                                   " of the run's barcodes but the matrix has " + std::to_string(now.total_cells) + " cells");
            if (n_before_doublets != now.total_cells)  // (the new cells' lines must follow the matrix' last cell)
                die(EXIT_PANIC, "the run's barcodes are " + std::to_string(n_before_doublets) + " lines but the matrix has " +
                                    std::to_string(now.total_cells) + " cells");
            const cellector_status st = cellector_add_doublets(g.c, dbl_a.data(), dbl_b.data(), dbl_a.size(), params.doublet_downsample_rate,
                                                               params.seed);
            if (st == CELLECTOR_EINVAL)  // (a summed count above 65535: the library names pair, locus and allele)
                die(1, "error: --doublets " + *params.doublets + ": " + cellector_last_error(g.c));
            g.ck(st, "add_doublets");
        }
        g.ck(cellector_ingest_finish(g.c, params.min_alt, params.min_ref), "load_cell_data");
    }
    lap("load_mtx (text -> device)");
    cellector_dims_t dm;
    g.ck(cellector_dims(g.c, &dm), "dims");
    const uint64_t N = dm.total_cells, L = dm.loci_used;
    if (barcodes.size() < N || ground_truth.size() < N)  // init_cell_data indexes both (load_data.rs:231-232)
        die(EXIT_PANIC, "index out of bounds: the barcodes file has " + std::to_string(barcodes.size()) +
                            " lines but the matrix has " + std::to_string(N) + " cells");
    std::vector<uint64_t> locus_ids(L);
    std::vector<uint32_t> entries_per_cell(N);
    g.ck(cellector_locus_ids(g.c, locus_ids.data()), "locus_ids");
    g.ck(cellector_entries_per_cell(g.c, entries_per_cell.data()), "entries_per_cell");

    if (params.initial_minority) {  // excluded_cells before the first compute_new_excluded
        std::vector<uint8_t> flags(N, 0);
        for (const uint32_t cell : initial_minority) {
            if (cell >= N)
                die(1, "error: --initial_minority: barcode '" + std::string(barcodes[cell]) + "' is line " + std::to_string(cell + 1) +
                           " of the barcodes file but the matrix has " + std::to_string(N) + " cells");
            flags[cell] = 1;
        }
        g.ck(cellector_set_excluded(g.c, flags.data()), "initial_minority");
        lap("initial exclusion set");
    }

    // load_vcf_data (load_data.rs:37-63)
    std::vector<VcfLocus> vcf_data;
    if (params.vcf) {
        Lines in(*params.vcf);
        std::string line;
        while (in.next(line)) {
            if (!line.empty() && line[0] == '#') continue;
            auto t = split(line, '\t');
            if (t.size() < 5) die(EXIT_PANIC, "index out of bounds: vcf record with fewer than 5 columns: " + line);
            vcf_data.push_back({t[0], t[1]});
        }
    }

    // cellector() (main.rs:36-50)
    std::vector<double> ll(N), ell(N), nloci(N), norm(N), var(params.zscore ? N : 0);
    std::vector<double> c_min(L), c_maj(L);
    const bool lx = params.locus_expected;
    std::vector<double> e_min(lx ? L : 0), e_maj(lx ? L : 0), v_min(lx ? L : 0), v_maj(lx ? L : 0);
    std::vector<uint64_t> n_min(L), n_maj(L), a_min(L), r_min(L), a_maj(L), r_maj(L);
    const std::string &od = params.output_directory;
    for (uint64_t iteration = 0;; iteration++) {
        cellector_iter_summary s;
        g.ck(cellector_em_iteration(g.c, params.interquartile_range_multiple, &s), "compute_new_excluded");
        printf("detected %llu new anomylous cells and rescued %llu cells to the majority in iteration %llu\n",
               (unsigned long long)s.n_new_excluded, (unsigned long long)s.n_rescued, (unsigned long long)(iteration + 1));
        printf("median normalized log likelihood %s with interquartile range %s, threshold %s\n", fmt(s.median).c_str(),
               fmt(s.iqr).c_str(), fmt(s.threshold).c_str());
        if (s.n_near_threshold && !params.resolve_near_ties && !params.resolve_assignments)  // stderr only: stdout stays byte-compatible with main.rs:338-339
            fprintf(stderr, "warning: iteration %llu: %llu cell(s) within 1e-9 (relative) of the threshold %s; the device's "
                            "log-pmf arithmetic differs from the reference's by ~1e-11, so their anomaly flag may differ from "
                            "the reference's\n", (unsigned long long)(iteration + 1), (unsigned long long)s.n_near_threshold,
                    fmt(s.threshold).c_str());
        g.ck(cellector_iter_cell_outputs(g.c, ll.data(), ell.data(), nloci.data(), norm.data()), "cell outputs");
        if (params.zscore) g.ck(cellector_iter_cell_variances(g.c, var.data()), "cell variances");
        g.ck(cellector_iter_locus_outputs(g.c, c_min.data(), c_maj.data(), n_min.data(), n_maj.data(), a_min.data(),
                                          r_min.data(), a_maj.data(), r_maj.data()), "locus outputs");
        if (lx) g.ck(cellector_iter_locus_moments(g.c, e_min.data(), e_maj.data(), v_min.data(), v_maj.data()), "locus moments");
        {   // locus_filter_and_output_locus_data (main.rs:422-498)
            FILE *f = create(od + "/iteration_" + std::to_string(iteration) + "_locus_contribution.tsv");
            fputs("locus_id\tchrom\tpos\tlog_likelihood_minority\tlog_likelihood_majority\texpected_loglike_minority\t"
                  "expected_loglike_majority\tminority_cellcount\tmajority_cellcount\tlog_likelihood_minority_per_cell\t"
                  "log_likelihood_majority_per_cell\tminority_alt\tminority_ref\tmajority_alt\tmajority_ref\tminority_af\t"
                  "majority_af", f);
            fputs(lx ? "\tvariance_minority\tvariance_majority\tzscore_minority\tzscore_majority\n" : "\n", f);
            std::vector<double> pc_min(L), pc_maj(L), for_thr;
            for (uint64_t l = 0; l < L; l++) {
                if (n_min[l]) { pc_min[l] = c_min[l] / (double)n_min[l]; for_thr.push_back(pc_min[l]); } else pc_min[l] = 0.0;
                pc_maj[l] = n_maj[l] ? c_maj[l] / (double)n_maj[l] : 0.0;
            }
            std::vector<size_t> order(L);
            std::iota(order.begin(), order.end(), (size_t)0);
            std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return pc_min[a] < pc_min[b]; });
            const double med = median_of(for_thr);
            for (uint64_t l = 0; l < L; l++)
                if (pc_min[l] < -80.0)  // main.rs:444-449; the mask itself was updated on the device
                    printf("filtering locus %llu locus index %llu because it was contributing %s vs median %s per cell to "
                           "log likelihood of minority cells\n", (unsigned long long)locus_ids[l], (unsigned long long)l,
                           fmt(pc_min[l]).c_str(), fmt(med).c_str());
            if (params.vcf)
                for (uint64_t l = 0; l < L; l++)
                    if (locus_ids[l] >= vcf_data.size()) die(EXIT_PANIC, "index out of bounds: vcf has fewer records than loci");
            write_rows(f, L, [&](uint64_t i, std::string &o) {
                const size_t l = order[i];
                const double af_min = a_min[l] + r_min[l] ? (double)a_min[l] / (double)(a_min[l] + r_min[l]) : 0.0;
                const double af_maj = a_maj[l] + r_maj[l] ? (double)a_maj[l] / (double)(a_maj[l] + r_maj[l]) : 0.0;
                put(o, locus_ids[l]); o += '\t';
                if (params.vcf) { o += vcf_data[locus_ids[l]].chrom; o += '\t'; o += vcf_data[locus_ids[l]].pos; }
                else o += "na\tna";
                o += '\t'; put(o, c_min[l]); o += '\t'; put(o, c_maj[l]);
                if (lx) { o += '\t'; put(o, e_min[l]); o += '\t'; put(o, e_maj[l]); }  // the sums main.rs:394 meant to form
                else { o += '\t'; put(o, c_min[l]); o += '\t'; put(o, c_maj[l]); }  // quirk Q6: "expected" == plain contribution
                o += '\t'; put(o, n_min[l]); o += '\t'; put(o, n_maj[l]);
                o += '\t'; put(o, pc_min[l]); o += '\t'; put(o, pc_maj[l]);
                o += '\t'; put(o, a_min[l]); o += '\t'; put(o, r_min[l]); o += '\t'; put(o, a_maj[l]); o += '\t'; put(o, r_maj[l]);
                o += '\t'; put(o, af_min); o += '\t'; put(o, af_maj);
                if (lx) {  // the z-score of main.rs:317-322 on the locus side: 0 without cells of the class or without variance
                    const double z_min = n_min[l] && v_min[l] > 0.0 ? (c_min[l] - e_min[l]) / std::sqrt(v_min[l]) : 0.0;
                    const double z_maj = n_maj[l] && v_maj[l] > 0.0 ? (c_maj[l] - e_maj[l]) / std::sqrt(v_maj[l]) : 0.0;
                    o += '\t'; put(o, v_min[l]); o += '\t'; put(o, v_maj[l]); o += '\t'; put(o, z_min); o += '\t'; put(o, z_maj);
                }
                o += '\n';
            });
            fclose(f);
        }
        {   // output_iteration_tsv (main.rs:349-366)
            FILE *f = create(od + "/iteration_" + std::to_string(iteration) + ".tsv");
            fputs(params.zscore ? "cell_id\tbarcode\tassignment\tlog_likelihood\texpected_log_likelihood\tnum_loci_used\texpected_log_variance\n"
                                : "cell_id\tbarcode\tassignment\tlog_likelihood\texpected_log_likelihood\tnum_loci_used\n", f);
            write_rows(f, N, [&](uint64_t c, std::string &o) {
                put(o, c); o += '\t'; o += barcodes[c]; o += '\t'; o += ground_truth[c];
                o += '\t'; put(o, ll[c]); o += '\t'; put(o, ell[c]); o += '\t'; put(o, nloci[c]);
                if (params.zscore) { o += '\t'; put(o, var[c]); }
                o += '\n';
            });
            fclose(f);
            f = create(od + "/iteration_" + std::to_string(iteration) + "_threshold.tsv");
            fputs(fmt(s.threshold).c_str(), f);
            fclose(f);
        }
        if (!s.any_change) break;
    }

    lap("EM loop + iteration files");
    // calculate_posteriors (main.rs:228-280)
    std::vector<double> posterior(N), doublet(N), ll_maj(N), ll_min(N);
    std::vector<uint8_t> excluded(N);
    std::vector<uint8_t> lib_label;  // --resolve_assignments: labels (codes of cellector_assign) and quals from the library
    std::vector<uint64_t> lib_qual;
    if (params.resolve_assignments) {
        lib_label.resize(N);
        lib_qual.resize(N);
        g.ck(cellector_assign(g.c, params.posterior_threshold, params.min_loci_used, posterior.data(), doublet.data(), ll_maj.data(),
                              ll_min.data(), lib_label.data(), nullptr, lib_qual.data()), "calculate_posteriors");
    } else
        g.ck(cellector_posteriors(g.c, posterior.data(), doublet.data(), ll_maj.data(), ll_min.data()), "calculate_posteriors");
    g.ck(cellector_excluded(g.c, excluded.data()), "excluded");
    lap("posteriors");

    // output_final_vcf (main.rs:52-131)
    if (params.vcf) {
        const uint64_t TL = dm.total_loci;
        std::vector<uint64_t> amin(TL), rmin(TL), amaj(TL), rmaj(TL);
        g.ck(cellector_final_allele_tallies(g.c, amin.data(), rmin.data(), amaj.data(), rmaj.data()), "load_mtx_final");
        FILE *f = create(od + "/cellector.vcf");
        const double ambient = 0.03, gt_thr = 0.99;
        const VcfLines v = read_vcf_lines(*params.vcf, TL);
        write_rows(f, v.lines.size(), [&](uint64_t i, std::string &o) {
            const std::string &ln = v.lines[i];
            if (v.rec_of[i] == VcfLines::META) { o += ln; o += '\n'; return; }
            if (v.rec_of[i] == VcfLines::CHROM) { o += ln; o += "\tmajority\tminority\n"; return; }
            const uint64_t r_ = v.rec_of[i];
            const GenotypeLocus g = genotype_locus(amin[r_] + amaj[r_], rmin[r_] + rmaj[r_], ambient);
            const GenotypeCall maj = genotype_call(g, amaj[r_], rmaj[r_], gt_thr), min = genotype_call(g, amin[r_], rmin[r_], gt_thr);
            o += ln; o += "\tGT:GP:AO:RO\t";
            o += genotype_string(maj.gt); o += ':'; put(o, maj.gp); o += ':'; put(o, amaj[r_]); o += ':'; put(o, rmaj[r_]); o += '\t';
            o += genotype_string(min.gt); o += ':'; put(o, min.gp); o += ':'; put(o, amin[r_]); o += ':'; put(o, rmin[r_]); o += '\n';
        });
        fclose(f);
    }

    lap("final tallies + cellector.vcf");
    // --cell_detail (main.rs:176: "TODO add detailed output for incorrectly assigned cells"): the PMFData of the listed cells
    // (main.rs:527-539) at every locus of the matrix — under the alpha / beta the loop ended with, `used` = the final loci
    // mask, the three value columns "na" at a locus the filter masked — and each entry's log-pmf under the three distributions
    // of calculate_posteriors, whose mask is all-true (main.rs:303).  Cells in file order, entries in the by-cell CSR's order.
    if (params.cell_detail) {
        for (const uint32_t cell : detail_cells)
            if (cell >= N)
                die(1, "error: --cell_detail: barcode '" + std::string(barcodes[cell]) + "' is line " + std::to_string(cell + 1) +
                           " of the barcodes file but the matrix has " + std::to_string(N) + " cells");
        if (params.vcf)
            for (uint64_t l = 0; l < L; l++)
                if (locus_ids[l] >= vcf_data.size()) die(EXIT_PANIC, "index out of bounds: vcf has fewer records than loci");
        std::vector<uint8_t> used(L);
        std::vector<double> alpha(L), beta(L), pa(L), pb(L);
        g.ck(cellector_loci_mask(g.c, used.data()), "loci_mask");
        g.ck(cellector_alpha_betas(g.c, alpha.data(), beta.data()), "alpha_betas");
        const uint64_t nc = detail_cells.size();
        std::vector<uint64_t> rec_ptr(nc + 1, 0);
        g.ck(cellector_cell_pmfs(g.c, alpha.data(), beta.data(), nullptr, detail_cells.data(), nc, rec_ptr.data(), 0, nullptr, nullptr,
                                 nullptr, nullptr, nullptr, nullptr), "cell_detail");
        const uint64_t nr = rec_ptr[nc];
        std::vector<uint32_t> li(nr), alt(nr), ref(nr);
        std::vector<double> lp(nr), elp(nr), var(nr), lp3[3];
        g.ck(cellector_cell_pmfs(g.c, alpha.data(), beta.data(), nullptr, detail_cells.data(), nc, rec_ptr.data(), nr, li.data(), alt.data(),
                                 ref.data(), lp.data(), elp.data(), var.data()), "cell_detail");
        for (int w = 0; w < 3; w++) {
            lp3[w].resize(nr);
            g.ck(cellector_posterior_alpha_betas(g.c, w, pa.data(), pb.data()), "posterior_alpha_betas");
            g.ck(cellector_cell_pmfs(g.c, pa.data(), pb.data(), nullptr, detail_cells.data(), nc, rec_ptr.data(), nr, nullptr, nullptr, nullptr,
                                     lp3[w].data(), nullptr, nullptr), "cell_detail");
        }
        std::vector<uint32_t> cell_of(nr);
        for (uint64_t j = 0; j < nc; j++)
            for (uint64_t i = rec_ptr[j]; i < rec_ptr[j + 1]; i++) cell_of[i] = detail_cells[j];
        FILE *f = create(od + "/cell_detail.tsv");
        fputs("cell_id\tbarcode\tlocus_id\tchrom\tpos\talt\tref\tused\talpha\tbeta\tlog_pmf\texpected_log_pmf\texpected_log_variance\t"
              "minority_log_pmf\tmajority_log_pmf\tdoublet_log_pmf\n", f);
        write_rows(f, nr, [&](uint64_t i, std::string &o) {
            const uint32_t c = cell_of[i], l = li[i];
            put(o, (uint64_t)c); o += '\t'; o += barcodes[c]; o += '\t'; put(o, locus_ids[l]); o += '\t';
            if (params.vcf) { o += vcf_data[locus_ids[l]].chrom; o += '\t'; o += vcf_data[locus_ids[l]].pos; }
            else o += "na\tna";
            o += '\t'; put(o, (uint64_t)alt[i]); o += '\t'; put(o, (uint64_t)ref[i]); o += '\t'; o += used[l] ? '1' : '0';
            o += '\t'; put(o, alpha[l]); o += '\t'; put(o, beta[l]);
            if (used[l]) { o += '\t'; put(o, lp[i]); o += '\t'; put(o, elp[i]); o += '\t'; put(o, var[i]); }
            else o += "\tna\tna\tna";
            for (int w = 0; w < 3; w++) { o += '\t'; put(o, lp3[w][i]); }
            o += '\n';
        });
        fclose(f);
        lap("cell_detail.tsv");
    }
    // output_final_assignments (main.rs:133-174)
    std::map<std::string, std::map<std::string, uint64_t>> assignment_gt_counts;
    std::map<std::string, uint64_t> gt_counts;
    {
        FILE *f = create(od + "/cellector_assignments.tsv");
        fputs("barcode\tposterior_assignment\tanomally_assignment\tlog_likelihood_loci_normalized\tloci_used\t"
              "posterior_assign_qual\tmajority_log_likelihood\tminority_log_likelihood\tground_truth_assignment\n", f);
        static const char *const PA[4] = {"unassigned", "0", "1", "doublet"};
        std::vector<uint8_t> pa_of(N);
        for (uint64_t c = 0; c < N; c++) {
            int pa = 0;
            if (posterior[c] > params.posterior_threshold) pa = 1;
            else if (1.0 - posterior[c] > params.posterior_threshold) pa = 2;
            if (doublet[c] > 0.5) pa = 3;
            if (entries_per_cell[c] < params.min_loci_used) pa = 0;  // quirk Q5
            if (!lib_label.empty()) pa = (lib_label[c] + 1) & 3;  // "0", "1", "doublet", "unassigned" -> PA's order
            pa_of[c] = (uint8_t)pa;
            assignment_gt_counts[PA[pa]][ground_truth[c]]++;
            gt_counts[ground_truth[c]]++;
        }
        write_rows(f, N, [&](uint64_t c, std::string &o) {
            const double post = std::fmax(posterior[c], 1.0 - posterior[c]);
            double q = std::fmin(-10.0 * std::log10(1.0 - post), 255.0);  // f64::min ignores NaN
            uint64_t qual = (q != q || q < 0.0) ? 0 : (uint64_t)q;          // `as usize` saturates
            if (!lib_qual.empty()) qual = lib_qual[c];
            o += barcodes[c]; o += '\t'; o += PA[pa_of[c]]; o += '\t'; o += excluded[c] ? "0" : "1";
            o += '\t'; put(o, norm[c]); o += '\t'; put(o, (uint64_t)nloci[c]); o += '\t'; put(o, qual);
            o += '\t'; put(o, ll_maj[c]); o += '\t'; put(o, ll_min[c]); o += '\t'; o += ground_truth[c]; o += '\n';
        });
        fclose(f);
    }
    lap("assignments file");
    {   // pretty_print (main.rs:177-226); ties in the count sort are in hash order there, by name here
        std::vector<std::pair<std::string, uint64_t>> cv(gt_counts.begin(), gt_counts.end());
        std::stable_sort(cv.begin(), cv.end(), [](const auto &a, const auto &b) { return a.second > b.second; });
        const std::string first_header = "cellector assignment   ", header = "      0      1      unassigned\n";
        std::string sb = first_header + header;
        size_t xoffset = std::max<size_t>(3, first_header.size() + 2);
        sb += "cell_hashing";
        sb += std::string(xoffset >= 12 ? xoffset - 12 : 0, ' ') + "|" + std::string(header.size() - 1, '-') + "|\n";
        auto get = [&](const char *k, const std::string &gt) -> uint64_t {
            auto it = assignment_gt_counts.find(k);
            if (it == assignment_gt_counts.end()) return 0;
            auto jt = it->second.find(gt);
            return jt == it->second.end() ? 0 : jt->second;
        };
        for (auto &[gt, cnt] : cv) {
            (void)cnt;
            xoffset = std::max(xoffset, gt.size() + 3);
            const std::string c0 = fmt(get("0", gt)), c1 = fmt(get("1", gt)), un = fmt(get("unassigned", gt));
            sb += gt;
            const size_t glen = gt.size() ? gt.size() - 1 : 0;
            sb += std::string(xoffset >= glen ? xoffset - glen : 0, ' ');
            sb += " |  " + c0 + std::string(c0.size() < 4 ? 4 - c0.size() : 0, ' ');
            sb += " |  " + c1 + std::string(c1.size() < 4 ? 4 - c1.size() : 0, ' ');
            sb += " |  " + un + std::string(un.size() < 12 ? 12 - un.size() : 0, ' ') + "|\n";
        }
        sb += std::string(xoffset, ' ') + "|" + std::string(header.size() - 1, '-') + "|\n";
        printf("\n\n%s\n", sb.c_str());
    }
    // --cluster: K genotype clusters of the matrix the run ended on, without labels; with one of the class flags they become the
    // classes of the block below
    if (params.cluster) {
        const uint32_t K = (uint32_t)params.cluster;
        const uint32_t R = params.cluster_restarts ? (uint32_t)params.cluster_restarts : std::min<uint32_t>(16, 64 / K);
        std::vector<uint8_t> lmask;
        if (params.cluster_mask_loop) {
            lmask.resize(dm.loci_used);
            g.ck(cellector_loci_mask(g.c, lmask.data()), "loci_mask");
        }
        std::vector<uint8_t> lab(N);
        std::vector<double> kll((uint64_t)K * N), kpost((uint64_t)K * N), obj(R);
        cellector_cluster_summary cs;
        g.ck(cellector_cluster(g.c, K, R, params.seed, nullptr, params.cluster_mask_loop ? lmask.data() : nullptr, lab.data(), kll.data(),
                               kpost.data(), nullptr, obj.data(), &cs), "cluster");
        std::string msg = "cluster: restart " + std::to_string(cs.best_restart) + " of " + std::to_string(R) + ", " +
                          std::to_string(cs.iterations) + " iterations, cluster sizes";
        for (uint32_t k = 0; k < K; k++) msg += " " + std::to_string(k) + "=" + std::to_string(cs.cluster_cells[k]);
        msg += " unassigned=" + std::to_string(cs.n_unlabelled);
        fprintf(stderr, "%s\n", msg.c_str());
        FILE *f = create(od + "/cellector_clusters.tsv");
        std::string head = "barcode\tcluster";
        for (uint32_t k = 0; k < K; k++) head += "\tposterior_" + std::to_string(k);
        for (uint32_t k = 0; k < K; k++) head += "\tlog_likelihood_" + std::to_string(k);
        head += '\n';
        fputs(head.c_str(), f);
        write_rows(f, N, [&](uint64_t c, std::string &o) {
            o += barcodes[c]; o += '\t';
            if (lab[c] == 255) o += "unassigned";
            else put(o, (uint64_t)lab[c]);
            for (uint32_t k = 0; k < K; k++) { o += '\t'; put(o, kpost[(uint64_t)k * N + c]); }
            for (uint32_t k = 0; k < K; k++) { o += '\t'; put(o, kll[(uint64_t)k * N + c]); }
            o += '\n';
        });
        fclose(f);
        lap("cellector_clusters.tsv");
        class_label = lab;
        class_names.clear();
        for (uint32_t k = 0; k < K; k++) class_names.push_back(std::to_string(k));
    }
    // --classes / --refine_classes: the K-class posteriors of every cell under the file's labelling (or --cluster's), refined one step
    // at a time so that every step gets its stderr line; then the scoring of the labelling in force
    if (params.classes || (params.cluster && (params.refine_classes || params.class_doublets || params.class_genotypes))) {
        const uint32_t K = (uint32_t)class_names.size();
        std::vector<uint8_t> lab(class_label.begin(), class_label.begin() + N), in_lab = lab, best(N);
        const bool dbl = params.class_doublets;
        std::vector<uint8_t> held(dbl ? N : 0, 0), call(dbl ? N : 0), bpair(dbl ? 2 * N : 0);
        std::vector<double> dpost(dbl ? N : 0);
        for (uint64_t it = 0; it < params.refine_classes; it++) {
            cellector_refine_summary rs;
            std::string tail;
            if (dbl) {  // the held-out refine: the called doublets (doublet posterior > 0.5) stay out of every tally
                cellector_refine_doublets_summary ds;
                g.ck(cellector_refine_class_doublets(g.c, lab.data(), held.data(), K, nullptr, nullptr, nullptr, nullptr, nullptr, 0.5, 1, 1, &ds,
                                                     nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), "refine_class_doublets");
                rs.n_moved_last = ds.n_moved_last;
                rs.converged = ds.converged;
                for (uint32_t k = 0; k < K; k++) rs.class_cells[k] = ds.class_cells[k];
                tail = " held=" + std::to_string(ds.n_held);
            } else
                g.ck(cellector_refine_classes(g.c, lab.data(), K, nullptr, nullptr, nullptr, 1, 1, &rs, nullptr, nullptr, nullptr), "refine_classes");
            std::string msg = "refine_classes step " + std::to_string(it + 1) + ": moved " + std::to_string(rs.n_moved_last) + ", class sizes";
            for (uint32_t k = 0; k < K; k++) msg += " " + class_names[k] + "=" + std::to_string(rs.class_cells[k]);
            msg += tail;
            fprintf(stderr, "%s\n", msg.c_str());
            if (rs.converged) break;
        }
        std::vector<double> cll((uint64_t)K * N), cpost((uint64_t)K * N);
        std::vector<uint64_t> cqual(N);
        if (dbl)
            g.ck(cellector_class_doublets(g.c, lab.data(), held.data(), K, nullptr, nullptr, nullptr, nullptr, nullptr, cll.data(), nullptr,
                                          cpost.data(), dpost.data(), best.data(), bpair.data(), call.data(), cqual.data()), "class_doublets");
        else
            g.ck(cellector_class_posteriors(g.c, lab.data(), K, nullptr, nullptr, nullptr, cll.data(), cpost.data(), best.data(), cqual.data()),
                 "class_posteriors");
        FILE *f = create(od + "/cellector_classes.tsv");
        std::string head = "barcode\tinput_label\tclass_assignment\tqual";
        for (uint32_t k = 0; k < K; k++) head += "\tlog_likelihood_" + class_names[k];
        for (uint32_t k = 0; k < K; k++) head += "\tposterior_" + class_names[k];
        if (dbl) head += "\tdoublet_posterior\tdoublet_pair";
        head += '\n';
        fputs(head.c_str(), f);
        write_rows(f, N, [&](uint64_t c, std::string &o) {
            const bool assigned = cpost[(uint64_t)best[c] * N + c] > params.posterior_threshold && entries_per_cell[c] >= params.min_loci_used;
            o += barcodes[c]; o += '\t'; o += in_lab[c] == 255 ? "na" : class_names[in_lab[c]].c_str(); o += '\t';
            // (main.rs:150-153: the doublet call overrides the label, and too few loci override both)
            const bool doublet = dbl && call[c] && entries_per_cell[c] >= params.min_loci_used;
            o += doublet ? "doublet" : assigned ? class_names[best[c]].c_str() : "unassigned"; o += '\t'; put(o, cqual[c]);
            for (uint32_t k = 0; k < K; k++) { o += '\t'; put(o, cll[(uint64_t)k * N + c]); }
            for (uint32_t k = 0; k < K; k++) { o += '\t'; put(o, cpost[(uint64_t)k * N + c]); }
            if (dbl) {
                o += '\t'; put(o, dpost[c]); o += '\t';
                if (bpair[2 * c] == 255) o += "na";
                else { o += class_names[bpair[2 * c]]; o += '+'; o += class_names[bpair[2 * c + 1]]; }
            }
            o += '\n';
        });
        fclose(f);
        lap("cellector_classes.tsv");
        class_label = lab;  // (--donors names the classes of the labelling in force)
        // --class_genotypes: a cell counts in the class its class_assignment names; doublet and unassigned cells are in none
        if (params.class_genotypes) {
            const uint64_t TL = dm.total_loci;
            std::vector<uint8_t> glab(N);
            for (uint64_t c = 0; c < N; c++) {
                const bool assigned = cpost[(uint64_t)best[c] * N + c] > params.posterior_threshold && entries_per_cell[c] >= params.min_loci_used;
                const bool doublet = dbl && call[c] && entries_per_cell[c] >= params.min_loci_used;
                glab[c] = !doublet && assigned ? best[c] : 255;
            }
            // (a run that assigned no cell to any class ends here with the library's refusal: all classes are dead)
            std::vector<uint64_t> galt((uint64_t)(K + 1) * TL), gref((uint64_t)(K + 1) * TL);
            g.ck(cellector_class_genotypes(g.c, glab.data(), K, 0.03, 0.99, nullptr, galt.data(), gref.data(), nullptr, nullptr, nullptr),
                 "class_genotypes");
            const double ambient = 0.03, gt_thr = 0.99;
            const VcfLines v = read_vcf_lines(*params.vcf, TL);
            std::vector<uint8_t> gts((uint64_t)K * TL, 0);  // by locus, for the concordance (a locus without a record: no call)
            FILE *fv = create(od + "/cellector_classes.vcf");
            write_rows(fv, v.lines.size(), [&](uint64_t i, std::string &o) {
                const std::string &ln = v.lines[i];
                if (v.rec_of[i] == VcfLines::META) { o += ln; o += '\n'; return; }
                if (v.rec_of[i] == VcfLines::CHROM) {
                    o += ln;
                    for (uint32_t k = 0; k < K; k++) { o += '\t'; o += class_names[k]; }
                    o += '\n';
                    return;
                }
                const uint64_t t = v.rec_of[i];
                uint64_t A = 0, R = 0;
                for (uint32_t k = 0; k <= K; k++) { A += galt[(uint64_t)k * TL + t]; R += gref[(uint64_t)k * TL + t]; }
                const GenotypeLocus gl = genotype_locus(A, R, ambient);
                o += ln; o += "\tGT:GP:AO:RO";
                for (uint32_t k = 0; k < K; k++) {
                    const uint64_t a = galt[(uint64_t)k * TL + t], r = gref[(uint64_t)k * TL + t];
                    const GenotypeCall q = genotype_call(gl, a, r, gt_thr);
                    gts[(uint64_t)k * TL + t] = q.gt;
                    o += '\t'; o += genotype_string(q.gt); o += ':'; put(o, q.gp); o += ':'; put(o, a); o += ':'; put(o, r);
                }
                o += '\n';
            });
            fclose(fv);
            FILE *fc = create(od + "/cellector_class_concordance.tsv");
            fputs("class_a\tclass_b\tboth_called\tdiscordant\n", fc);
            for (uint32_t a = 0; a < K; a++)
                for (uint32_t b = a + 1; b < K; b++) {
                    uint64_t both = 0, disc = 0;
                    for (uint64_t t = 0; t < TL; t++) {
                        const uint8_t x = gts[(uint64_t)a * TL + t], y = gts[(uint64_t)b * TL + t];
                        both += x && y;
                        disc += x && y && x != y;
                    }
                    fprintf(fc, "%s\t%s\t%llu\t%llu\n", class_names[a].c_str(), class_names[b].c_str(), (unsigned long long)both,
                            (unsigned long long)disc);
                }
            fclose(fc);
            lap("cellector_classes.vcf");
        }
    }
    // --donors: every cell against the genotyped donors of the pool, and the classes in force (--classes / --cluster, refined if asked)
    // named by donor
    if (params.donors) {
        DonorGenotypes dg;
        const bool soft = params.donor_field != "GT";
        if (soft) dg.field = params.donor_field;
        {
            Lines vin(*params.vcf);
            std::string line;
            while (vin.next(line)) dg.add_variant_line(line);
            Lines din(*params.donors);
            while (din.next(line)) dg.add_donor_line(line);
        }
        const uint32_t D = (uint32_t)dg.names.size();
        if (D < 1 || D > 64) die(1, "error: --donors " + *params.donors + ": " + std::to_string(dg.names.size()) + " sample columns, 1..64 donors are supported");
        if (dg.total_loci != dm.total_loci)
            die(1, "error: --donors: --vcf " + *params.vcf + " has " + std::to_string(dg.total_loci) + " records but the matrix has " +
                       std::to_string(dm.total_loci) + " loci");
        cellector_donor_params dp;
        cellector_donor_default_params(&dp);
        dp.err = params.donor_error; dp.ambient = params.donor_ambient; dp.doublet_rate = params.donor_doublet_rate;
        dp.posterior_threshold = params.posterior_threshold;
        dp.min_loci = std::max<uint64_t>(params.min_loci_used, 1);
        std::vector<double> dll((uint64_t)N * D), dpost((uint64_t)N * D), dppost((uint64_t)N * D), ddbl(N);
        std::vector<uint8_t> dbest(N), dsecond(N), dpair(N), dstatus(N);
        std::vector<uint32_t> dn(N);
        cellector_donor_summary ds;
        // --donor_field GP / GL / PL: the soft calls score the weights; what needs a hard call takes every row's most probable genotype
        const std::vector<uint8_t> hard_gt = soft ? donor_hard_codes(dg.gp) : std::vector<uint8_t>();
        const uint8_t *const gt_codes = soft ? hard_gt.data() : dg.gt.data();
        auto donor_pass = [&]() {
            if (soft)
                g.ck(cellector_donor_posteriors_gp(g.c, dg.gp.data(), D, &dp, nullptr, nullptr, nullptr, dll.data(), nullptr, dpost.data(),
                                                   dppost.data(), ddbl.data(), dbest.data(), dsecond.data(), dpair.data(), dn.data(),
                                                   dstatus.data(), nullptr, &ds, nullptr, nullptr), "donor_posteriors_gp");
            else
                g.ck(cellector_donor_posteriors(g.c, dg.gt.data(), D, &dp, nullptr, nullptr, nullptr, dll.data(), nullptr, dpost.data(),
                                                dppost.data(), ddbl.data(), dbest.data(), dsecond.data(), dpair.data(), dn.data(), dstatus.data(),
                                                nullptr, &ds, nullptr, nullptr), "donor_posteriors");
            fprintf(stderr, "donors: %u donors, singlet=%llu doublet=%llu ambiguous=%llu unassigned=%llu\n", D,
                    (unsigned long long)ds.n_singlet, (unsigned long long)ds.n_doublet, (unsigned long long)ds.n_ambiguous,
                    (unsigned long long)ds.n_unassigned);
        };
        donor_pass();
        // --estimate_ambient: the pool's ambient fraction from the singlets, each under its best donor; apply: the donors again with it
        if (params.estimate_ambient) {
            std::vector<uint8_t> assign(N);
            for (uint64_t c = 0; c < N; c++) assign[c] = dstatus[c] == 0 ? dbest[c] : (uint8_t)255;
            cellector_ambient_params ap;
            cellector_ambient_default_params(&ap);
            ap.err = params.donor_error;
            cellector_ambient_summary as;
            std::vector<double> crho(N), cse(N);
            std::vector<uint32_t> cn(N);
            g.ck(cellector_estimate_ambient(g.c, gt_codes, D, assign.data(), &ap, nullptr, &as, crho.data(), cse.data(), cn.data()),
                 "estimate_ambient");
            {
                std::string o = "ambient: rho=";
                put(o, as.rho); o += " se="; put(o, as.se); o += " cells="; put(o, as.n_cells_used);
                o += as.at_boundary ? " at_boundary=1\n" : " at_boundary=0\n";
                fputs(o.c_str(), stdout);
            }
            FILE *fa = create(od + "/cellector_ambient.tsv");
            fputs("source\tcells\trho\tse\n", fa);
            {
                std::string o = "pool\t";
                put(o, as.n_cells_used); o += '\t'; put(o, as.rho); o += '\t'; put(o, as.se); o += '\n';
                for (uint32_t d = 0; d < D; d++) {
                    o += dg.names[d]; o += '\t'; put(o, as.source_cells[d]); o += '\t';
                    if (as.source_cells[d]) { put(o, as.source_rho[d]); o += '\t'; put(o, as.source_se[d]); }
                    else o += "NA\tNA";
                    o += '\n';
                }
                fputs(o.c_str(), fa);
            }
            fclose(fa);
            FILE *fc = create(od + "/cellector_ambient_cells.tsv");
            fputs("barcode\tdonor\tn_loci\trho\tse\n", fc);
            write_rows(fc, N, [&](uint64_t c, std::string &o) {
                o += barcodes[c]; o += '\t';
                if (assign[c] == 255) { o += "NA\tNA\tNA\tNA\n"; return; }
                o += dg.names[assign[c]]; o += '\t'; put(o, (uint64_t)cn[c]); o += '\t';
                if (crho[c] != crho[c]) o += "NA\tNA";
                else { put(o, crho[c]); o += '\t'; put(o, cse[c]); }
                o += '\n';
            });
            fclose(fc);
            lap("cellector_ambient.tsv");
            if (params.estimate_ambient == 2) {
                dp.ambient = as.rho;
                donor_pass();
            }
        }
        FILE *f = create(od + "/cellector_donors.tsv");
        std::string head = "barcode\tstatus\tdonor\tsecond_donor\tbest_pair\tposterior\tpair_posterior\tdoublet_posterior\tn_loci";
        for (uint32_t d = 0; d < D; d++) head += "\tlog_likelihood_" + dg.names[d];
        head += '\n';
        fputs(head.c_str(), f);
        write_rows(f, N, [&](uint64_t c, std::string &o) {
            static const char *const STATUS[3] = {"singlet", "doublet", "ambiguous"};
            const uint8_t b = dbest[c];
            o += barcodes[c]; o += '\t'; o += dstatus[c] < 3 ? STATUS[dstatus[c]] : "unassigned"; o += '\t';
            o += dg.names[b]; o += '\t';
            o += dsecond[c] == 255 ? "na" : dg.names[dsecond[c]].c_str(); o += '\t';
            if (dpair[c] == 255) o += "na";
            else { o += dg.names[b]; o += '+'; o += dg.names[dpair[c]]; }
            o += '\t'; put(o, dpost[c * D + b]);
            o += '\t'; put(o, dpair[c] == 255 ? 0.0 : dppost[c * D + dpair[c]]);
            o += '\t'; put(o, ddbl[c]);
            o += '\t'; put(o, (uint64_t)dn[c]);
            for (uint32_t d = 0; d < D; d++) { o += '\t'; put(o, dll[c * D + d]); }
            o += '\n';
        });
        fclose(f);
        lap("cellector_donors.tsv");
        // --donor_fit: the fit of the called hypothesis under the hard calls and the parameters the donor pass ended with
        if (params.donor_fit) {
            cellector_donor_fit_params fp;
            cellector_donor_fit_default_params(&fp);
            if (params.donor_fit_iqr) fp.iqr_multiple = *params.donor_fit_iqr;
            std::vector<double> fe((uint64_t)N * D), fv((uint64_t)N * D), fpe((uint64_t)N * D), fpv((uint64_t)N * D), fll((uint64_t)N * D),
                fpll((uint64_t)N * D), fz(N);
            std::vector<uint8_t> ha(N), hb(N), fstatus(N), unmatched(N);
            std::vector<uint32_t> fn(N);
            cellector_donor_fit_summary fs;
            g.ck(cellector_donor_fit(g.c, gt_codes, D, &dp, &fp, nullptr, nullptr, nullptr, fe.data(), fv.data(), fpe.data(), fpv.data(), nullptr,
                                     nullptr, fz.data(), ha.data(), hb.data(), fstatus.data(), unmatched.data(), &fs, nullptr, nullptr),
                 "donor_fit");
            // the sums of the called hypothesis: the hard call's own ll and pair_ll (the bits the fit took its z from)
            g.ck(cellector_donor_posteriors(g.c, gt_codes, D, &dp, nullptr, nullptr, nullptr, fll.data(), fpll.data(), nullptr, nullptr, nullptr,
                                            nullptr, nullptr, nullptr, fn.data(), nullptr, nullptr, nullptr, nullptr, nullptr),
                 "donor_posteriors");
            {
                std::string o = "donor_fit: keys=";
                put(o, fs.n_keys); o += " median="; put(o, fs.median); o += " iqr="; put(o, fs.iqr); o += " threshold="; put(o, fs.threshold);
                o += " unmatched="; put(o, fs.n_unmatched); o += '\n';
                fputs(o.c_str(), stdout);
            }
            FILE *ff = create(od + "/cellector_donor_fit.tsv");
            fputs("barcode\tstatus\tdonor\tsecond_donor\tn_loci\tll\texpected\tvariance\tz\tunmatched\n", ff);
            write_rows(ff, N, [&](uint64_t c, std::string &o) {
                static const char *const STATUS[3] = {"singlet", "doublet", "ambiguous"};
                o += barcodes[c]; o += '\t'; o += fstatus[c] < 3 ? STATUS[fstatus[c]] : "unassigned"; o += '\t';
                if (fstatus[c] == 255) {
                    o += "NA\tNA\t"; put(o, (uint64_t)fn[c]); o += "\tNA\tNA\tNA\tNA\tNA\n";
                    return;
                }
                const bool pair = hb[c] != 255;
                const uint64_t at = c * D + (pair ? hb[c] : ha[c]);
                o += dg.names[ha[c]]; o += '\t'; o += pair ? dg.names[hb[c]].c_str() : "NA"; o += '\t'; put(o, (uint64_t)fn[c]);
                o += '\t'; put(o, pair ? fpll[at] : fll[at]);
                o += '\t'; put(o, pair ? fpe[at] : fe[at]);
                o += '\t'; put(o, pair ? fpv[at] : fv[at]);
                o += '\t'; put(o, fz[c]);
                o += unmatched[c] ? "\t1\n" : "\t0\n";
            });
            fclose(ff);
            lap("cellector_donor_fit.tsv");
        }
        if (params.classes || params.cluster) {
            const uint32_t K = (uint32_t)class_names.size();
            std::vector<uint8_t> lab(class_label.begin(), class_label.begin() + N), mbest(K);
            std::vector<double> mll((uint64_t)K * D), margin(K);
            std::vector<uint64_t> mcells(K);
            if (soft)
                g.ck(cellector_match_donors_gp(g.c, lab.data(), K, dg.gp.data(), D, &dp, nullptr, mll.data(), mbest.data(), margin.data(),
                                               mcells.data()), "match_donors_gp");
            else
                g.ck(cellector_match_donors(g.c, lab.data(), K, dg.gt.data(), D, &dp, nullptr, mll.data(), mbest.data(), margin.data(), mcells.data()),
                     "match_donors");
            FILE *fm = create(od + "/cellector_cluster_donors.tsv");
            std::string mh = "class\tcells\tdonor\tmargin";
            for (uint32_t d = 0; d < D; d++) mh += "\tlog_likelihood_" + dg.names[d];
            mh += '\n';
            fputs(mh.c_str(), fm);
            for (uint32_t k = 0; k < K; k++) {
                std::string o = class_names[k];
                o += '\t'; put(o, mcells[k]); o += '\t'; o += mbest[k] == 255 ? "na" : dg.names[mbest[k]].c_str(); o += '\t'; put(o, margin[k]);
                for (uint32_t d = 0; d < D; d++) { o += '\t'; put(o, mll[(uint64_t)k * D + d]); }
                o += '\n';
                fputs(o.c_str(), fm);
            }
            fclose(fm);
            lap("cellector_cluster_donors.tsv");
        }
    }
    // Every output file is closed: leave without tearing the context down.  Handing ~150 GB of device memory back block
    // by block (and destroying the host vectors) was half a second of the 1M x 200k run; the driver reclaims a dead
    // process' memory in one go.
    fflush(stdout);
    fflush(stderr);
    // (a multi-device ctx always leaves the orderly way: its communicator and worker threads are torn down in order;
    //  so does a run under a profiler or leak checker, CELLECTOR_TEARDOWN=1)
    if (devices.size() > 1 || getenv("CELLECTOR_TEARDOWN")) {
        cellector_destroy(g.c);
        return 0;
    }
    _exit(0);
}
