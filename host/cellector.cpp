// cellector — host binary of the MI355X build: same command line (cellector/src/params.yml), same input files
// and the same output files as the reference's Rust binary (main.rs), with the scoring path running in
// libcellector_hip.so through the C ABI of include/cellector_ffi.h.  The reference host is Rust; this image has no
// Rust toolchain, so the host above the C ABI is C++ (INTEGRATION.md shows the equivalent Rust binding).
//
// Host-side pieces restated here (cited per function): load_params (main.rs:629-677; cli_params.h), create_output_dir /
// load_barcodes / load_ground_truth / load_vcf_data (load_data.rs:37-107), the driver loop cellector()
// (main.rs:36-50), the writers output_iteration_tsv (main.rs:349-366), locus_filter_and_output_locus_data
// (main.rs:422-498), output_final_assignments + pretty_print (main.rs:133-226), output_final_vcf (main.rs:52-131).
//
// main() at the end of the file is the run's table of contents: read_inputs (every input file but the matrices and the
// VCFs, before a device is opened), open_device, load_matrix, then one stage per phase.  A stage takes the Run record and
// exactly the earlier results it reads, and returns what a later one reads.
#include <sys/stat.h>
#include <unistd.h>

#include <chrono>
#include <map>
#include <memory>
#include <numeric>

#include "../include/cellector_ffi.h"
#include "cli_params.h"
#include "donor_vcf_host.h"
#include "genotype_host.h"
#include "host_text.h"

namespace {

// ---- the run's barcodes -----------------------------------------------------------------------------------------
// A flat open-addressing table over views into the barcodes file, which is read whole — a
// std::unordered_map<std::string, size_t> of a million barcodes was 0.3-0.6 s of node allocations.
struct BarcodeIndex {
    std::vector<uint32_t> slot;  // line index + 1 of the LAST line with that barcode, 0 = empty
    size_t n_distinct = 0;
    // the slot that holds key, or the empty one where it would go
    size_t probe(const std::vector<std::string_view> &names, std::string_view key) const
    {
        const size_t cap = slot.size();
        size_t h = std::hash<std::string_view>{}(key) & (cap - 1);
        while (slot[h] && names[slot[h] - 1] != key) h = (h + 1) & (cap - 1);
        return h;
    }
    void build(const std::vector<std::string_view> &names)
    {
        n_distinct = 0;
        size_t cap = 16;
        while (cap < 2 * names.size() + 2) cap <<= 1;
        slot.assign(cap, 0u);
        if (names.size() >= 0xffffffffull) die(EXIT_PANIC, "too many barcodes");
        for (size_t i = 0; i < names.size(); i++) {
            const size_t h = probe(names, names[i]);
            if (!slot[h]) n_distinct++;
            slot[h] = (uint32_t)i + 1;  // (a later duplicate overwrites an earlier one: HashMap::insert)
        }
    }
    size_t find(const std::vector<std::string_view> &names, std::string_view key) const  // SIZE_MAX: not among them
    {
        if (slot.empty()) return SIZE_MAX;
        const size_t h = probe(names, key);
        return slot[h] ? slot[h] - 1 : SIZE_MAX;
    }
};

// load_barcodes (load_data.rs:73-83): the lines of the file; barcode -> cell index for the ground truth, a later
// duplicate overwriting an earlier one.  --cells, --mix_* and --doublets each turn the list into what the barcodes file
// of their run would hold; `whole` keeps the file as it was to name a barcode that --cells dropped.
struct CellNames {
    std::unique_ptr<const std::string> text;  // the barcodes file (on the heap: the views outlive a move of this record)
    std::vector<std::string_view> names;      // the run's cells, by cell index
    std::vector<std::string> mix_names;       // owned: the renamed barcodes of --mix_*'s cells
    std::vector<std::string> dbl_names;       // owned: <A>+<B> of --doublets' cells
    BarcodeIndex index;
    std::vector<std::string_view> whole;      // with --cells: every line of the file
    BarcodeIndex whole_index;

    size_t size() const { return names.size(); }
    std::string_view operator[](size_t cell) const { return names[cell]; }
    void reindex() { index.build(names); }
    size_t find(std::string_view name) const { return index.find(names, name); }
    bool dropped_by_cells(std::string_view name) const { return whole_index.find(whole, name) != SIZE_MAX; }
};

// a barcode list file: one barcode per line, the first tab-separated column, blank lines ignored; each(line_no, barcode)
template <class F>
void for_each_listed_barcode(const std::string &path, F each)
{
    Lines in(path);
    std::string line;
    for (size_t line_no = 1; in.next(line); line_no++) {
        const std::string bc = line.substr(0, line.find('\t'));
        if (!bc.empty()) each(line_no, bc);
    }
}

// the labelling in force for the class stages: --classes' file, then --cluster's clusters, then --refine_classes' result
struct ClassLabels {
    std::vector<uint8_t> label;  // per cell, 255 = unlabelled
    std::vector<std::string> names;
};

// what the input files say, before a device is opened
struct RunInputs {
    CellNames cells;
    std::vector<uint32_t> kept_lines;        // --cells: the line index of every kept barcode, ascending
    size_t mix_lines = 0;                    // --mix_barcodes: its lines ...
    std::vector<uint8_t> mix_keep;           // ... and with --mix_cells, which of them are taken
    size_t n_before_doublets = 0;            // the cells --doublets' new ones follow
    std::vector<uint32_t> dbl_a, dbl_b;      // --doublets: the pairs' parents
    std::vector<std::string> ground_truth;   // one label per DISTINCT barcode
    std::vector<uint32_t> initial_minority;  // --initial_minority: the cells the loop starts from as excluded_cells (main.rs:37 has `HashSet::new()`)
    std::vector<uint32_t> detail_cells;      // --cell_detail: the cells whose per-locus records are written after the posterior phase
    ClassLabels classes;                     // --classes
};

// --cells: from here on the barcodes file IS its listed lines, in its own order: the ground truth, the barcode lists of the
// other flags and every output see only them, exactly as on a filtered barcodes.tsv.  The matrix follows after the load
// (cellector_restage)
void keep_listed_cells(const Params &params, RunInputs &in)
{
    CellNames &cells = in.cells;
    std::vector<uint8_t> listed(cells.size(), 0);
    for_each_listed_barcode(*params.cells, [&](size_t line_no, const std::string &bc) {
        const size_t cell = cells.find(bc);
        if (cell == SIZE_MAX)
            die(1, "error: --cells " + *params.cells + " line " + std::to_string(line_no) + ": barcode '" + bc +
                       "' is not in the barcodes file " + params.barcodes);
        listed[cell] = 1;
    });
    for (size_t i = 0; i < listed.size(); i++)
        if (listed[i]) in.kept_lines.push_back((uint32_t)i);
    if (in.kept_lines.empty()) die(1, "error: --cells " + *params.cells + " lists no barcode");
    cells.whole = cells.names;
    cells.whole_index = cells.index;
    cells.names.clear();
    for (const uint32_t i : in.kept_lines) cells.names.push_back(cells.whole[i]);
    cells.reindex();
}

// --mix_*: the second dataset's barcodes (those --mix_cells lists, in their file's order) follow the first one's, the last
// character replaced by 2 (combiner/src/main.rs:174-184); from here on the barcodes file IS that list, as the combiner
// writes it into its output's barcodes.tsv
void append_mix_cells(const Params &params, RunInputs &in)
{
    const std::string mix_text = read_whole(*params.mix_barcodes);
    const std::vector<std::string_view> theirs = split_lines(mix_text);
    in.mix_lines = theirs.size();
    if (params.mix_cells) {
        std::map<std::string_view, size_t> line_of;  // (a later duplicate overwrites an earlier one, as load_barcodes)
        for (size_t i = 0; i < theirs.size(); i++) line_of[theirs[i]] = i;
        in.mix_keep.assign(theirs.size(), 0);
        for_each_listed_barcode(*params.mix_cells, [&](size_t line_no, const std::string &bc) {
            const auto at = line_of.find(std::string_view(bc));
            if (at == line_of.end())
                die(1, "error: --mix_cells " + *params.mix_cells + " line " + std::to_string(line_no) + ": barcode '" + bc +
                           "' is not in the barcodes file " + *params.mix_barcodes);
            in.mix_keep[at->second] = 1;
        });
        if (std::find(in.mix_keep.begin(), in.mix_keep.end(), 1) == in.mix_keep.end())
            die(1, "error: --mix_cells " + *params.mix_cells + " lists no barcode");
    }
    CellNames &cells = in.cells;
    for (size_t i = 0; i < theirs.size(); i++) {
        if (params.mix_cells && !in.mix_keep[i]) continue;
        std::string bc(theirs[i]);
        if (!bc.empty()) bc.pop_back();
        bc += '2';
        cells.mix_names.push_back(std::move(bc));
    }
    for (const std::string &bc : cells.mix_names) cells.names.push_back(bc);  // (mix_names is complete: the views stay valid)
    cells.reindex();
}

// --doublets: the pairs, by the names the cells carry now; the new cells <A>+<B> follow all others, and from here on the
// barcodes file IS that list.  The matrix follows after the load (cellector_add_doublets)
void append_doublets(const Params &params, RunInputs &in)
{
    CellNames &cells = in.cells;
    Lines file(*params.doublets);
    std::string line;
    std::map<std::string, size_t> seen;  // name -> line
    for (size_t line_no = 1; file.next(line); line_no++) {
        if (line.empty()) continue;
        const std::string where = "error: --doublets " + *params.doublets + " line " + std::to_string(line_no) + ": ";
        auto cols = split(line, '\t');
        if (cols.size() != 2 || cols[0].empty() || cols[1].empty())
            die(1, where + "two tab-separated barcodes expected, got '" + line + "'");
        size_t cell[2];
        for (int k = 0; k < 2; k++) {
            cell[k] = cells.find(cols[k]);
            if (cell[k] == SIZE_MAX)
                die(1, where + "barcode '" + cols[k] + "' is not among the run's cells (the barcodes file " + params.barcodes +
                           (params.cells ? " after --cells" : "") + (params.mix() ? ", then --mix_barcodes" : "") + ")");
        }
        if (cell[0] == cell[1]) die(1, where + "barcode '" + cols[0] + "' is paired with itself");
        std::string name = cols[0] + "+" + cols[1];
        const auto [at, fresh] = seen.emplace(name, line_no);
        if (!fresh)
            die(1, where + "the pair is line " + std::to_string(at->second) + " already: the cell '" + name + "' would exist twice");
        if (cells.find(name) != SIZE_MAX) die(1, where + "the run has a cell named '" + name + "' already");
        in.dbl_a.push_back((uint32_t)cell[0]);
        in.dbl_b.push_back((uint32_t)cell[1]);
        cells.dbl_names.push_back(std::move(name));
    }
    if (cells.dbl_names.empty()) die(1, "error: --doublets " + *params.doublets + " lists no pair");
    for (const std::string &bc : cells.dbl_names) cells.names.push_back(bc);  // (dbl_names is complete: the views stay valid)
    cells.reindex();
}

// the combiner's barcodes.tsv and gt.tsv of the mixture (main.rs:155-186); without -g the run's ground truth.  With --doublets
// the cells there before keep the label in force (-g's, else the mixture's, else singlet) and the new ones are doublet
void write_run_barcodes_and_truth(const Params &params, RunInputs &in, size_t n_first)
{
    const CellNames &cells = in.cells;
    std::vector<std::string> &ground_truth = in.ground_truth;
    std::string bc_out, gt_out;
    for (size_t i = 0; i < cells.size(); i++) {
        std::string label = i >= in.n_before_doublets ? "doublet" : params.mix() ? (i < n_first ? "majority" : "minority") : "singlet";
        const size_t cell = cells.find(cells[i]);
        if (params.doublets && params.ground_truth && cell < ground_truth.size()) {  // -g's label; a new cell it does not name stays doublet
            if (i < in.n_before_doublets || ground_truth[cell] != "na") label = ground_truth[cell];
        }
        bc_out += cells[i]; bc_out += '\n';
        gt_out += cells[i]; gt_out += '\t'; gt_out += label; gt_out += '\n';
        if ((!params.ground_truth || i >= in.n_before_doublets) && cell < ground_truth.size()) ground_truth[cell] = label;
    }
    // an input of this run under one of the two names in the output directory would be lost: refuse before either is written
    for (const char *name : {"barcodes.tsv", "gt.tsv"}) {
        const std::string path = params.output_directory + "/" + name;
        struct stat mine, theirs;
        if (stat(path.c_str(), &mine) != 0) continue;
        for (const auto &[flag, file] : std::vector<std::pair<const char *, std::optional<std::string>>>{
                 {"--barcodes", params.barcodes}, {"--ground_truth", params.ground_truth}, {"--mix_barcodes", params.mix_barcodes},
                 {"--mix_cells", params.mix_cells}, {"--cells", params.cells}, {"--doublets", params.doublets},
                 {"--initial_minority", params.initial_minority},
                 {"--cell_detail", params.cell_detail}})
            if (file && stat(file->c_str(), &theirs) == 0 && mine.st_dev == theirs.st_dev && mine.st_ino == theirs.st_ino)
                die(1, std::string(params.mix() ? "error: the mixture's " : "error: the run's ") + name + " would overwrite the " + flag + " file " + *file +
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

// --write_matrices: the two names the matrix goes under (cellector_write_mtx or, with --write_matrices_gz, cellector_write_mtx_bgzf,
// after the load)
std::pair<const char *, const char *> written_matrix_names(const Params &params)
{
    if (params.write_matrices_gz)
        return params.write_matrices - 1 == CELLECTOR_WRITE_DEPTH ? std::make_pair("ad.mtx.gz", "dp.mtx.gz") : std::make_pair("alt.mtx.gz", "ref.mtx.gz");
    return params.write_matrices - 1 == CELLECTOR_WRITE_DEPTH ? std::make_pair("ad.mtx", "dp.mtx") : std::make_pair("alt.mtx", "ref.mtx");
}

// --write_matrices, before a device is opened and before anything is written: an input of this run under one of the names the
// flag writes in the output directory would be lost
void refuse_to_overwrite_inputs_with_matrices(const Params &params)
{
    const auto [first, second] = written_matrix_names(params);
    const bool own_barcodes = !params.mix() && !params.doublets;
    std::vector<const char *> names{first, second};
    if (own_barcodes) names.push_back("barcodes.tsv");
    for (const char *name : names) {
        const std::string path = params.output_directory + "/" + name;
        struct stat mine, theirs;
        if (stat(path.c_str(), &mine) != 0) continue;
        for (const auto &[flag, file] : std::vector<std::pair<const char *, std::optional<std::string>>>{
                 {"--alt", params.alt_mtx}, {"--ref", params.ref_mtx}, {"--mix_alt", params.mix_alt}, {"--mix_ref", params.mix_ref},
                 {"--vcf", params.vcf}, {"--barcodes", params.barcodes}, {"--ground_truth", params.ground_truth},
                 {"--mix_barcodes", params.mix_barcodes}, {"--mix_cells", params.mix_cells}, {"--cells", params.cells},
                 {"--doublets", params.doublets}, {"--initial_minority", params.initial_minority}, {"--cell_detail", params.cell_detail},
                 {"--classes", params.classes}, {"--donors", params.donors}})
            if (file && stat(file->c_str(), &theirs) == 0 && mine.st_dev == theirs.st_dev && mine.st_ino == theirs.st_ino)
                die(1, std::string("error: --write_matrices' ") + name + " would overwrite the " + flag + " file " + *file +
                           ": choose another --output_directory");
    }
}

// ... then barcodes.tsv of the cells in force, where --mix_* / --doublets have not written it already
void write_barcodes_beside_matrices(const Params &params, const RunInputs &in)
{
    if (params.mix() || params.doublets) return;
    std::string text;
    for (size_t i = 0; i < in.cells.size(); i++) { text += in.cells[i]; text += '\n'; }
    const std::string path = params.output_directory + "/barcodes.tsv";
    FILE *f = fopen(path.c_str(), "w");
    if (!f) die(EXIT_PANIC, "Unable to create file " + path);
    fwrite(text.data(), 1, text.size(), f);
    fclose(f);
}

// a barcode list of an extension flag: one per line, first tab-separated column, blank lines ignored; file order, repeats kept
std::vector<uint32_t> read_barcode_list(const Params &params, const CellNames &names, const char *flag, const std::string &path)
{
    std::vector<uint32_t> cells;
    for_each_listed_barcode(path, [&](size_t line_no, const std::string &bc) {
        const size_t cell = names.find(bc);
        if (cell == SIZE_MAX && names.dropped_by_cells(bc))
            die(1, std::string("error: --") + flag + " " + path + " line " + std::to_string(line_no) + ": barcode '" + bc +
                       "' is not among the cells --cells " + *params.cells + " keeps");
        if (cell == SIZE_MAX)
            die(1, std::string("error: --") + flag + " " + path + " line " + std::to_string(line_no) + ": barcode '" + bc +
                       "' is not in the barcodes file " + params.barcodes);
        cells.push_back((uint32_t)cell);
    });
    return cells;
}

// --classes: barcode<TAB>label, parsed like load_ground_truth (load_data.rs:85-107): a line without exactly two columns is an
// error, a barcode the run does not have is ignored, a later line of a barcode replaces an earlier one.  Labels are numbered by
// first appearance; a cell no line names is unlabelled (255)
ClassLabels read_classes(const std::string &path, const CellNames &cells)
{
    ClassLabels classes;
    classes.label.assign(cells.index.n_distinct, 255);
    Lines in(path);
    std::string line;
    while (in.next(line)) {
        auto cols = split(line, '\t');
        if (cols.size() != 2) die(EXIT_PANIC, "Invalid line format: " + line + "\nThe correct format is: barcode\tlabel");
        size_t k = std::find(classes.names.begin(), classes.names.end(), cols[1]) - classes.names.begin();
        if (k == classes.names.size()) {
            if (k == 16) die(1, "error: --classes " + path + ": more than 16 distinct labels ('" + cols[1] + "' is the 17th)");
            classes.names.push_back(cols[1]);
        }
        const size_t cell = cells.find(cols[0]);
        if (cell != SIZE_MAX && cell < classes.label.size()) classes.label[cell] = (uint8_t)k;
    }
    if (classes.names.empty()) die(1, "error: --classes " + path + ": no label");
    return classes;
}

// Everything that happens before a device is opened; no library call.  A bad input file is refused here, with exit 1 and
// its message, before the GPU is touched.
RunInputs read_inputs(const Params &params)
{
    // create_output_dir (load_data.rs:66-71): non-recursive mkdir, failure ignored (quirk Q13)
    (void)mkdir(params.output_directory.c_str(), 0777);

    RunInputs in;
    CellNames &cells = in.cells;
    cells.text = std::make_unique<const std::string>(read_whole(params.barcodes));
    cells.names = split_lines(*cells.text);
    cells.reindex();
    if (params.cells) keep_listed_cells(params, in);
    const size_t n_first = cells.size();
    if (params.mix()) append_mix_cells(params, in);
    in.n_before_doublets = cells.size();
    if (params.doublets) append_doublets(params, in);

    // load_ground_truth (load_data.rs:85-107): one label per DISTINCT barcode (the vector has the map's length)
    in.ground_truth.assign(cells.index.n_distinct, "na");
    if (params.ground_truth) {
        Lines file(*params.ground_truth);
        std::string line;
        while (file.next(line)) {
            auto cols = split(line, '\t');
            if (cols.size() != 2) die(EXIT_PANIC, "Invalid line format: " + line + "\nThe correct format is: barcode\tassignment");
            const size_t cell = cells.find(cols[0]);
            if (cell != SIZE_MAX && cell < in.ground_truth.size()) in.ground_truth[cell] = cols[1];
        }
    }
    if (params.write_matrices) refuse_to_overwrite_inputs_with_matrices(params);
    if (params.mix() || params.doublets) write_run_barcodes_and_truth(params, in, n_first);
    if (params.write_matrices) write_barcodes_beside_matrices(params, in);

    if (params.initial_minority) in.initial_minority = read_barcode_list(params, cells, "initial_minority", *params.initial_minority);
    if (params.cell_detail) in.detail_cells = read_barcode_list(params, cells, "cell_detail", *params.cell_detail);
    if (params.classes) in.classes = read_classes(*params.classes, cells);
    return in;
}

// ---- the run ----------------------------------------------------------------------------------------------------
struct Ctx {
    cellector_ctx *c = nullptr;
    void ck(cellector_status s, const char *what) const
    {
        if (s != CELLECTOR_OK) die(EXIT_PANIC, std::string(what) + ": " + (c ? cellector_last_error(c) : "no context"));
    }
};

// CELLECTOR_TIMING=1: phase wall times on stderr (not part of the reference's output)
struct Lap {
    const bool timing = getenv("CELLECTOR_TIMING") != nullptr;
    mutable std::chrono::steady_clock::time_point t_prev = std::chrono::steady_clock::now();
    void operator()(const char *what) const
    {
        const auto now = std::chrono::steady_clock::now();
        if (timing) fprintf(stderr, "[timing] %-24s %8.3f s\n", what, std::chrono::duration<double>(now - t_prev).count());
        t_prev = now;
    }
};

struct VcfLocus { std::string chrom, pos; };

// what every stage after the inputs reads
struct Run {
    const Params &params;
    RunInputs in;
    Lap lap;
    Ctx g;
    std::vector<int> devices;
    cellector_dims_t dims{};
    uint64_t N = 0, L = 0;  // cells, used loci
    std::vector<uint64_t> locus_ids;
    std::vector<uint32_t> entries_per_cell;
    std::vector<VcfLocus> vcf_data;  // with --vcf: chrom and pos of every record
    Run(const Params &p, RunInputs &&inputs) : params(p), in(std::move(inputs)) {}
    std::string out(const char *name) const { return params.output_directory + "/" + name; }
};

// load_cell_data (load_data.rs:134-181) on the device
// Which GPUs: --device n / --devices a,b,... as given; neither (cellector_pipeline.py:223-226 passes neither flag): GPU 0 —
// the multi-GPU path over RCCL is opt-in until it has run on a multi-GPU node (README).  --devices auto: all visible GPUs
// when the input is large enough to feed them (one GPU per 4 GB of alt.mtx text, i.e. >= 1.3e8 entries each: below that
// the per-iteration exchanges and the communicator set-up cost more than the extra GPUs save); should the multi-device
// ctx fail to come up there, the run falls back to GPU 0 with a note on stderr.
Ctx open_device(const Params &params, std::vector<int> &devices)
{
    Ctx g;
    devices = params.devices;
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
    if (params.gz_device) g.ck(cellector_set_option(g.c, "gz_device", 1), "gz_device");
    return g;
}

// a listed cell the matrix does not reach: `flag`'s barcode is line cell + 1 `of_what`
void check_cell_in_matrix(const char *flag, std::string_view barcode, uint64_t cell, const char *of_what, uint64_t matrix_cells)
{
    if (cell >= matrix_cells)
        die(1, std::string("error: --") + flag + ": barcode '" + std::string(barcode) + "' is line " + std::to_string(cell + 1) + " " + of_what +
                   " but the matrix has " + std::to_string(matrix_cells) + " cells");
}

// a pair's entries staged: zipped line by line, the reference's reading, or under --matrix_pair join | depth joined by (locus, cell)
cellector_status ingest_pair(const Params &params, cellector_ctx *c, const std::string &first, const std::string &second)
{
    if (!params.matrix_pair) return cellector_ingest_mtx(c, first.c_str(), second.c_str());
    cellector_join_summary s;
    const cellector_status st = cellector_ingest_mtx_joined(c, first.c_str(), second.c_str(), params.matrix_pair, &s);
    if (st == CELLECTOR_OK)
        fprintf(stderr, "matrix_pair %s: %llu entries of %s, %llu of %s: %llu keys in both, %llu only in the first, %llu only in the second, %llu staged\n",
                params.matrix_pair == CELLECTOR_JOIN_DEPTH ? "depth" : "join", (unsigned long long)s.n_first, first.c_str(),
                (unsigned long long)s.n_second, second.c_str(), (unsigned long long)s.n_both, (unsigned long long)s.n_first_only,
                (unsigned long long)s.n_second_only, (unsigned long long)s.n_out);
    return st;
}

// --mix_*: the second dataset, staged in a ctx of its own on the same GPU, merged in, released
void combine_second_dataset(const Run &run)
{
    const Params &params = run.params;
    const RunInputs &in = run.in;
    const Ctx &g = run.g;
    Ctx second;
    if (cellector_create(&second.c, run.devices[0]) != CELLECTOR_OK) die(EXIT_PANIC, "cellector: no second context on the device");
    if (params.gz_device) second.ck(cellector_set_option(second.c, "gz_device", 1), "gz_device");
    second.ck(ingest_pair(params, second.c, *params.mix_alt, *params.mix_ref), "load_cell_data (--mix_alt / --mix_ref)");
    cellector_dims_t ours, theirs;
    g.ck(cellector_dims(g.c, &ours), "dims");
    second.ck(cellector_dims(second.c, &theirs), "dims");
    if (ours.total_loci != theirs.total_loci)
        die(1, "error: --mix_alt " + *params.mix_alt + " has " + std::to_string(theirs.total_loci) + " loci, --alt " + params.alt_mtx +
                   " has " + std::to_string(ours.total_loci) + " loci: both datasets must come from the same variant VCF");
    if (in.mix_lines < theirs.total_cells)
        die(EXIT_PANIC, "index out of bounds: the barcodes file " + *params.mix_barcodes + " has " + std::to_string(in.mix_lines) +
                            " lines but the matrix has " + std::to_string(theirs.total_cells) + " cells");
    std::vector<uint8_t> take;
    if (params.mix_cells) {
        for (size_t i = theirs.total_cells; i < in.mix_keep.size(); i++)
            if (in.mix_keep[i])
                die(1, "error: --mix_cells: a listed barcode is line " + std::to_string(i + 1) + " of " + *params.mix_barcodes +
                           " but the matrix has " + std::to_string(theirs.total_cells) + " cells");
        take.assign(in.mix_keep.begin(), in.mix_keep.begin() + (ptrdiff_t)theirs.total_cells);
    } else if (in.mix_lines != theirs.total_cells) {
        die(EXIT_PANIC, "the barcodes file " + *params.mix_barcodes + " has " + std::to_string(in.mix_lines) + " lines but the matrix has " +
                            std::to_string(theirs.total_cells) + " cells");
    }
    g.ck(cellector_combine(g.c, second.c, params.mix_cells ? take.data() : nullptr, nullptr, ours.total_loci,
                           params.downsample_rate.value_or(0.0), params.seed), "combine");
    cellector_destroy(second.c);
}

// --doublets, last: the pairs name the cells as they are now
void add_doublets(const Run &run)
{
    const Params &params = run.params;
    const RunInputs &in = run.in;
    const Ctx &g = run.g;
    cellector_dims_t now;
    g.ck(cellector_dims(g.c, &now), "dims");
    for (size_t j = 0; j < in.dbl_a.size(); j++)
        for (const uint32_t cell : {in.dbl_a[j], in.dbl_b[j]})
            check_cell_in_matrix("doublets", run.in.cells[cell], cell, "of the run's barcodes", now.total_cells);
    if (in.n_before_doublets != now.total_cells)  // (the new cells' lines must follow the matrix' last cell)
        die(EXIT_PANIC, "the run's barcodes are " + std::to_string(in.n_before_doublets) + " lines but the matrix has " +
                            std::to_string(now.total_cells) + " cells");
    const cellector_status st = cellector_add_doublets(g.c, in.dbl_a.data(), in.dbl_b.data(), in.dbl_a.size(), params.doublet_downsample_rate,
                                                       params.seed);
    if (st == CELLECTOR_EINVAL)  // (a summed count above 65535: the library names pair, locus and allele)
        die(1, "error: --doublets " + *params.doublets + ": " + cellector_last_error(g.c));
    g.ck(st, "add_doublets");
}

// --write_matrices: the staged matrix as it is now, every flag that changes it applied, before the locus filter
void write_matrices(const Run &run)
{
    const Params &params = run.params;
    const auto [first, second] = written_matrix_names(params);
    const int mode = params.write_matrices - 1;
    cellector_write_summary s;
    cellector_write_bgzf_summary gz = {};
    if (params.write_matrices_gz) {
        run.g.ck(cellector_write_mtx_bgzf(run.g.c, run.out(first).c_str(), run.out(second).c_str(), mode, CELLECTOR_MTX_HEADER_ZERO, &gz),
                 "write_matrices");
        s = gz.text;
    } else {
        run.g.ck(cellector_write_mtx(run.g.c, run.out(first).c_str(), run.out(second).c_str(), mode, CELLECTOR_MTX_HEADER_ZERO, &s), "write_matrices");
    }
    fprintf(stderr, "write_matrices %s: %llu entries, %llu with alt = ref = 0%s: %llu lines, %llu bytes in %s; %llu lines, %llu bytes in %s; %llu windows",
            mode == CELLECTOR_WRITE_DEPTH ? "depth" : mode == CELLECTOR_WRITE_SPARSE ? "sparse" : "aligned", (unsigned long long)s.n_entries,
            (unsigned long long)s.n_dropped_keys, mode == CELLECTOR_WRITE_ALIGNED ? "" : " (in neither file)", (unsigned long long)s.lines_first,
            (unsigned long long)s.bytes_first, first, (unsigned long long)s.lines_second, (unsigned long long)s.bytes_second, second,
            (unsigned long long)s.n_windows);
    if (params.write_matrices_gz)  // (the bytes above are the text's)
        fprintf(stderr, "; compressed to %llu and %llu bytes in %llu and %llu blocks (%llu stored)", (unsigned long long)gz.file_bytes_first,
                (unsigned long long)gz.file_bytes_second, (unsigned long long)gz.blocks_first, (unsigned long long)gz.blocks_second,
                (unsigned long long)gz.stored_blocks);
    fputc('\n', stderr);
}

// the matrix onto the device — the direct load, or ingest, restage, combine, add-doublets and finish — and its shape
void load_matrix(Run &run)
{
    const Params &params = run.params;
    const RunInputs &in = run.in;
    const Ctx &g = run.g;
    if (!params.restage() && !params.mix() && !params.doublets && !params.matrix_pair && !params.write_matrices) {
        g.ck(cellector_load_mtx(g.c, params.alt_mtx.c_str(), params.ref_mtx.c_str(), params.min_alt, params.min_ref), "load_cell_data");
    } else if (!params.restage() && !params.mix() && !params.doublets) {
        g.ck(ingest_pair(params, g.c, params.alt_mtx, params.ref_mtx), "load_cell_data");
        if (params.write_matrices) write_matrices(run);
        g.ck(cellector_ingest_finish(g.c, params.min_alt, params.min_ref), "load_cell_data");
    } else {  // --cells / --downsample_rate: the staged matrix is cut and thinned on the device before the locus filter sees it
        g.ck(ingest_pair(params, g.c, params.alt_mtx, params.ref_mtx), "load_cell_data");
        cellector_dims_t staged;
        g.ck(cellector_dims(g.c, &staged), "dims");
        std::vector<uint8_t> keep;
        if (params.cells) {
            keep.assign(staged.total_cells, 0);
            for (const uint32_t i : in.kept_lines) {
                check_cell_in_matrix("cells", in.cells.whole[i], i, "of the barcodes file", staged.total_cells);
                keep[i] = 1;
            }
        }
        g.ck(cellector_restage(g.c, params.cells ? keep.data() : nullptr, params.downsample_rate.value_or(0.0), params.seed), "restage");
        if (params.cells) {  // the barcodes above were filtered by the same rule the library renumbers by: cellector_cell_origin says so
            std::vector<uint32_t> origin(in.kept_lines.size());
            g.ck(cellector_cell_origin(g.c, origin.data()), "cell_origin");
            if (origin != in.kept_lines) die(EXIT_PANIC, "--cells: the restaged cells are not the listed barcodes in file order");
        }
        if (params.mix()) combine_second_dataset(run);
        if (params.doublets) add_doublets(run);
        if (params.write_matrices) write_matrices(run);
        g.ck(cellector_ingest_finish(g.c, params.min_alt, params.min_ref), "load_cell_data");
    }
    run.lap("load_mtx (text -> device)");
    g.ck(cellector_dims(g.c, &run.dims), "dims");
    run.N = run.dims.total_cells;
    run.L = run.dims.loci_used;
    if (in.cells.size() < run.N || in.ground_truth.size() < run.N)  // init_cell_data indexes both (load_data.rs:231-232)
        die(EXIT_PANIC, "index out of bounds: the barcodes file has " + std::to_string(in.cells.size()) +
                            " lines but the matrix has " + std::to_string(run.N) + " cells");
    run.locus_ids.resize(run.L);
    run.entries_per_cell.resize(run.N);
    g.ck(cellector_locus_ids(g.c, run.locus_ids.data()), "locus_ids");
    g.ck(cellector_entries_per_cell(g.c, run.entries_per_cell.data()), "entries_per_cell");
}

// --initial_minority: excluded_cells before the first compute_new_excluded
void set_initial_minority(const Run &run)
{
    std::vector<uint8_t> flags(run.N, 0);
    for (const uint32_t cell : run.in.initial_minority) {
        check_cell_in_matrix("initial_minority", run.in.cells[cell], cell, "of the barcodes file", run.N);
        flags[cell] = 1;
    }
    run.g.ck(cellector_set_excluded(run.g.c, flags.data()), "initial_minority");
    run.lap("initial exclusion set");
}

// load_vcf_data (load_data.rs:37-63)
std::vector<VcfLocus> load_vcf_data(const std::string &path)
{
    std::vector<VcfLocus> vcf_data;
    Lines in(path);
    std::string line;
    while (in.next(line)) {
        if (!line.empty() && line[0] == '#') continue;
        auto t = split(line, '\t');
        if (t.size() < 5) die(EXIT_PANIC, "index out of bounds: vcf record with fewer than 5 columns: " + line);
        vcf_data.push_back({t[0], t[1]});
    }
    return vcf_data;
}
// the writers that name a locus by chrom and pos index vcf_data by locus id
void check_vcf_covers_loci(const Run &run)
{
    if (!run.params.vcf) return;
    for (uint64_t l = 0; l < run.L; l++)
        if (run.locus_ids[l] >= run.vcf_data.size()) die(EXIT_PANIC, "index out of bounds: vcf has fewer records than loci");
}
// the columns chrom<TAB>pos of used locus l
void put_chrom_pos(const Run &run, std::string &o, size_t l)
{
    if (run.params.vcf) { o += run.vcf_data[run.locus_ids[l]].chrom; o += '\t'; o += run.vcf_data[run.locus_ids[l]].pos; }
    else o += "na\tna";
}

// ---- cellector() (main.rs:36-50) ----------------------------------------------------------------------------------
struct LocusOutputs {
    std::vector<double> c_min, c_maj, e_min, e_maj, v_min, v_maj;  // (e_, v_: with --locus_expected)
    std::vector<uint64_t> n_min, n_maj, a_min, r_min, a_maj, r_maj;
    LocusOutputs(uint64_t L, bool moments)
        : c_min(L), c_maj(L), e_min(moments ? L : 0), e_maj(moments ? L : 0), v_min(moments ? L : 0), v_maj(moments ? L : 0), n_min(L),
          n_maj(L), a_min(L), r_min(L), a_maj(L), r_maj(L) {}
};
struct LoopResult {
    std::vector<double> ll, ell, nloci, norm, var;  // of the last iteration (var: with --normalization zscore)
};

// locus_filter_and_output_locus_data (main.rs:422-498)
void write_locus_contribution(const Run &run, uint64_t iteration, const LocusOutputs &lo)
{
    const uint64_t L = run.L;
    const bool lx = run.params.locus_expected;
    const std::vector<double> &c_min = lo.c_min, &c_maj = lo.c_maj, &e_min = lo.e_min, &e_maj = lo.e_maj, &v_min = lo.v_min, &v_maj = lo.v_maj;
    const std::vector<uint64_t> &n_min = lo.n_min, &n_maj = lo.n_maj, &a_min = lo.a_min, &r_min = lo.r_min, &a_maj = lo.a_maj, &r_maj = lo.r_maj;
    FILE *f = create(run.out("iteration_") + std::to_string(iteration) + "_locus_contribution.tsv");
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
                   "log likelihood of minority cells\n", (unsigned long long)run.locus_ids[l], (unsigned long long)l,
                   fmt(pc_min[l]).c_str(), fmt(med).c_str());
    check_vcf_covers_loci(run);
    write_rows(f, L, [&](uint64_t i, std::string &o) {
        const size_t l = order[i];
        const double af_min = a_min[l] + r_min[l] ? (double)a_min[l] / (double)(a_min[l] + r_min[l]) : 0.0;
        const double af_maj = a_maj[l] + r_maj[l] ? (double)a_maj[l] / (double)(a_maj[l] + r_maj[l]) : 0.0;
        put(o, run.locus_ids[l]); o += '\t';
        put_chrom_pos(run, o, l);
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

// output_iteration_tsv (main.rs:349-366)
void write_iteration_tsv(const Run &run, uint64_t iteration, const LoopResult &r, double threshold)
{
    const bool zscore = run.params.zscore;
    const CellNames &barcodes = run.in.cells;
    const std::vector<std::string> &ground_truth = run.in.ground_truth;
    write_tsv(run.out("iteration_") + std::to_string(iteration) + ".tsv",
              zscore ? "cell_id\tbarcode\tassignment\tlog_likelihood\texpected_log_likelihood\tnum_loci_used\texpected_log_variance\n"
                     : "cell_id\tbarcode\tassignment\tlog_likelihood\texpected_log_likelihood\tnum_loci_used\n",
              run.N, [&](uint64_t c, std::string &o) {
                  put(o, c); o += '\t'; o += barcodes[c]; o += '\t'; o += ground_truth[c];
                  o += '\t'; put(o, r.ll[c]); o += '\t'; put(o, r.ell[c]); o += '\t'; put(o, r.nloci[c]);
                  if (zscore) { o += '\t'; put(o, r.var[c]); }
                  o += '\n';
              });
    FILE *f = create(run.out("iteration_") + std::to_string(iteration) + "_threshold.tsv");
    fputs(fmt(threshold).c_str(), f);
    fclose(f);
}

LoopResult run_loop(const Run &run)
{
    const Params &params = run.params;
    const Ctx &g = run.g;
    const uint64_t N = run.N, L = run.L;
    LoopResult r{std::vector<double>(N), std::vector<double>(N), std::vector<double>(N), std::vector<double>(N),
                 std::vector<double>(params.zscore ? N : 0)};
    const bool lx = params.locus_expected;
    LocusOutputs lo(L, lx);
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
        g.ck(cellector_iter_cell_outputs(g.c, r.ll.data(), r.ell.data(), r.nloci.data(), r.norm.data()), "cell outputs");
        if (params.zscore) g.ck(cellector_iter_cell_variances(g.c, r.var.data()), "cell variances");
        g.ck(cellector_iter_locus_outputs(g.c, lo.c_min.data(), lo.c_maj.data(), lo.n_min.data(), lo.n_maj.data(), lo.a_min.data(),
                                          lo.r_min.data(), lo.a_maj.data(), lo.r_maj.data()), "locus outputs");
        if (lx) g.ck(cellector_iter_locus_moments(g.c, lo.e_min.data(), lo.e_maj.data(), lo.v_min.data(), lo.v_maj.data()), "locus moments");
        write_locus_contribution(run, iteration, lo);
        write_iteration_tsv(run, iteration, r, s.threshold);
        if (!s.any_change) break;
    }
    return r;
}

// ---- calculate_posteriors (main.rs:228-280) and the final files --------------------------------------------------
struct Posteriors {
    std::vector<double> posterior, doublet, ll_maj, ll_min;
    std::vector<uint8_t> excluded;
    std::vector<uint8_t> lib_label;  // --resolve_assignments: labels (codes of cellector_assign) and quals from the library
    std::vector<uint64_t> lib_qual;
};
Posteriors run_posteriors(const Run &run)
{
    const Params &params = run.params;
    const Ctx &g = run.g;
    const uint64_t N = run.N;
    Posteriors p{std::vector<double>(N), std::vector<double>(N), std::vector<double>(N), std::vector<double>(N), std::vector<uint8_t>(N), {}, {}};
    if (params.resolve_assignments) {
        p.lib_label.resize(N);
        p.lib_qual.resize(N);
        g.ck(cellector_assign(g.c, params.posterior_threshold, params.min_loci_used, p.posterior.data(), p.doublet.data(), p.ll_maj.data(),
                              p.ll_min.data(), p.lib_label.data(), nullptr, p.lib_qual.data()), "calculate_posteriors");
    } else
        g.ck(cellector_posteriors(g.c, p.posterior.data(), p.doublet.data(), p.ll_maj.data(), p.ll_min.data()), "calculate_posteriors");
    g.ck(cellector_excluded(g.c, p.excluded.data()), "excluded");
    return p;
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
// The input vcf with sample columns (main.rs:64-131): META lines are copied, sample_names(o) appends the names to the #CHROM
// line, and a record gets GT:GP:AO:RO and what samples(locus, o) appends, one column per sample
template <class Names, class Samples>
void write_sample_vcf(const Run &run, const char *name, Names sample_names, Samples samples)
{
    FILE *f = create(run.out(name));
    const VcfLines v = read_vcf_lines(*run.params.vcf, run.dims.total_loci);
    write_rows(f, v.lines.size(), [&](uint64_t i, std::string &o) {
        o += v.lines[i];
        if (v.rec_of[i] == VcfLines::CHROM) sample_names(o);
        else if (v.rec_of[i] != VcfLines::META) { o += "\tGT:GP:AO:RO"; samples(v.rec_of[i], o); }
        o += '\n';
    });
    fclose(f);
}
// one sample column of a record
void put_sample(std::string &o, const GenotypeCall &call, uint64_t alt, uint64_t ref)
{
    o += '\t'; o += genotype_string(call.gt); o += ':'; put(o, call.gp); o += ':'; put(o, alt); o += ':'; put(o, ref);
}
constexpr double VCF_AMBIENT = 0.03, VCF_GT_THRESHOLD = 0.99;  // main.rs:58-59, for both VCFs

// output_final_vcf (main.rs:52-131)
void write_final_vcf(const Run &run)
{
    const uint64_t TL = run.dims.total_loci;
    std::vector<uint64_t> amin(TL), rmin(TL), amaj(TL), rmaj(TL);
    run.g.ck(cellector_final_allele_tallies(run.g.c, amin.data(), rmin.data(), amaj.data(), rmaj.data()), "load_mtx_final");
    write_sample_vcf(run, "cellector.vcf", [](std::string &o) { o += "\tmajority\tminority"; }, [&](uint64_t t, std::string &o) {
        const GenotypeLocus g = genotype_locus(amin[t] + amaj[t], rmin[t] + rmaj[t], VCF_AMBIENT);
        put_sample(o, genotype_call(g, amaj[t], rmaj[t], VCF_GT_THRESHOLD), amaj[t], rmaj[t]);
        put_sample(o, genotype_call(g, amin[t], rmin[t], VCF_GT_THRESHOLD), amin[t], rmin[t]);
    });
}

// --cell_detail (main.rs:176: "TODO add detailed output for incorrectly assigned cells"): the PMFData of the listed cells
// (main.rs:527-539) at every locus of the matrix — under the alpha / beta the loop ended with, `used` = the final loci
// mask, the three value columns "na" at a locus the filter masked — and each entry's log-pmf under the three distributions
// of calculate_posteriors, whose mask is all-true (main.rs:303).  Cells in file order, entries in the by-cell CSR's order.
void write_cell_detail(const Run &run)
{
    const Ctx &g = run.g;
    const uint64_t L = run.L;
    const std::vector<uint32_t> &detail_cells = run.in.detail_cells;
    const CellNames &barcodes = run.in.cells;
    for (const uint32_t cell : detail_cells) check_cell_in_matrix("cell_detail", barcodes[cell], cell, "of the barcodes file", run.N);
    check_vcf_covers_loci(run);
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
    write_tsv(run.out("cell_detail.tsv"),
              "cell_id\tbarcode\tlocus_id\tchrom\tpos\talt\tref\tused\talpha\tbeta\tlog_pmf\texpected_log_pmf\texpected_log_variance\t"
              "minority_log_pmf\tmajority_log_pmf\tdoublet_log_pmf\n",
              nr, [&](uint64_t i, std::string &o) {
                  const uint32_t c = cell_of[i], l = li[i];
                  put(o, (uint64_t)c); o += '\t'; o += barcodes[c]; o += '\t'; put(o, run.locus_ids[l]); o += '\t';
                  put_chrom_pos(run, o, l);
                  o += '\t'; put(o, (uint64_t)alt[i]); o += '\t'; put(o, (uint64_t)ref[i]); o += '\t'; o += used[l] ? '1' : '0';
                  o += '\t'; put(o, alpha[l]); o += '\t'; put(o, beta[l]);
                  if (used[l]) { o += '\t'; put(o, lp[i]); o += '\t'; put(o, elp[i]); o += '\t'; put(o, var[i]); }
                  else o += "\tna\tna\tna";
                  for (int w = 0; w < 3; w++) { o += '\t'; put(o, lp3[w][i]); }
                  o += '\n';
              });
    run.lap("cell_detail.tsv");
}

// the counts of the confusion table: assignment -> ground truth -> cells, and ground truth -> cells
struct ConfusionCounts {
    std::map<std::string, std::map<std::string, uint64_t>> assignment_gt_counts;
    std::map<std::string, uint64_t> gt_counts;
};
// output_final_assignments (main.rs:133-174)
ConfusionCounts write_assignments(const Run &run, const LoopResult &loop, const Posteriors &p)
{
    const Params &params = run.params;
    const uint64_t N = run.N;
    const CellNames &barcodes = run.in.cells;
    const std::vector<std::string> &ground_truth = run.in.ground_truth;
    ConfusionCounts counts;
    static const char *const PA[4] = {"unassigned", "0", "1", "doublet"};
    std::vector<uint8_t> pa_of(N);
    for (uint64_t c = 0; c < N; c++) {
        int pa = 0;
        if (p.posterior[c] > params.posterior_threshold) pa = 1;
        else if (1.0 - p.posterior[c] > params.posterior_threshold) pa = 2;
        if (p.doublet[c] > 0.5) pa = 3;
        if (run.entries_per_cell[c] < params.min_loci_used) pa = 0;  // quirk Q5
        if (!p.lib_label.empty()) pa = (p.lib_label[c] + 1) & 3;  // "0", "1", "doublet", "unassigned" -> PA's order
        pa_of[c] = (uint8_t)pa;
        counts.assignment_gt_counts[PA[pa]][ground_truth[c]]++;
        counts.gt_counts[ground_truth[c]]++;
    }
    write_tsv(run.out("cellector_assignments.tsv"),
              "barcode\tposterior_assignment\tanomally_assignment\tlog_likelihood_loci_normalized\tloci_used\t"
              "posterior_assign_qual\tmajority_log_likelihood\tminority_log_likelihood\tground_truth_assignment\n",
              N, [&](uint64_t c, std::string &o) {
                  const double post = std::fmax(p.posterior[c], 1.0 - p.posterior[c]);
                  double q = std::fmin(-10.0 * std::log10(1.0 - post), 255.0);  // f64::min ignores NaN
                  uint64_t qual = (q != q || q < 0.0) ? 0 : (uint64_t)q;          // `as usize` saturates
                  if (!p.lib_qual.empty()) qual = p.lib_qual[c];
                  o += barcodes[c]; o += '\t'; o += PA[pa_of[c]]; o += '\t'; o += p.excluded[c] ? "0" : "1";
                  o += '\t'; put(o, loop.norm[c]); o += '\t'; put(o, (uint64_t)loop.nloci[c]); o += '\t'; put(o, qual);
                  o += '\t'; put(o, p.ll_maj[c]); o += '\t'; put(o, p.ll_min[c]); o += '\t'; o += ground_truth[c]; o += '\n';
              });
    return counts;
}

// pretty_print (main.rs:177-226); ties in the count sort are in hash order there, by name here
void print_confusion_table(const ConfusionCounts &counts)
{
    std::vector<std::pair<std::string, uint64_t>> cv(counts.gt_counts.begin(), counts.gt_counts.end());
    std::stable_sort(cv.begin(), cv.end(), [](const auto &a, const auto &b) { return a.second > b.second; });
    const std::string first_header = "cellector assignment   ", header = "      0      1      unassigned\n";
    std::string sb = first_header + header;
    size_t xoffset = std::max<size_t>(3, first_header.size() + 2);
    sb += "cell_hashing";
    sb += std::string(xoffset >= 12 ? xoffset - 12 : 0, ' ') + "|" + std::string(header.size() - 1, '-') + "|\n";
    auto get = [&](const char *k, const std::string &gt) -> uint64_t {
        auto it = counts.assignment_gt_counts.find(k);
        if (it == counts.assignment_gt_counts.end()) return 0;
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

// ---- --cluster, --classes -------------------------------------------------------------------------------------------
// --cluster: K genotype clusters of the matrix the run ended on, without labels; with one of the class flags they become the
// classes of run_classes
ClassLabels run_cluster(const Run &run)
{
    const Params &params = run.params;
    const Ctx &g = run.g;
    const uint64_t N = run.N;
    const CellNames &barcodes = run.in.cells;
    const uint32_t K = (uint32_t)params.cluster;
    const uint32_t R = params.cluster_restarts ? (uint32_t)params.cluster_restarts : std::min<uint32_t>(16, 64 / K);
    std::vector<uint8_t> lmask;
    if (params.cluster_mask_loop) {
        lmask.resize(run.dims.loci_used);
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
    std::string head = "barcode\tcluster";
    for (uint32_t k = 0; k < K; k++) head += "\tposterior_" + std::to_string(k);
    for (uint32_t k = 0; k < K; k++) head += "\tlog_likelihood_" + std::to_string(k);
    head += '\n';
    write_tsv(run.out("cellector_clusters.tsv"), head, N, [&](uint64_t c, std::string &o) {
        o += barcodes[c]; o += '\t';
        if (lab[c] == 255) o += "unassigned";
        else put(o, (uint64_t)lab[c]);
        for (uint32_t k = 0; k < K; k++) { o += '\t'; put(o, kpost[(uint64_t)k * N + c]); }
        for (uint32_t k = 0; k < K; k++) { o += '\t'; put(o, kll[(uint64_t)k * N + c]); }
        o += '\n';
    });
    run.lap("cellector_clusters.tsv");
    ClassLabels clusters{lab, {}};
    for (uint32_t k = 0; k < K; k++) clusters.names.push_back(std::to_string(k));
    return clusters;
}

// the scoring of a labelling: per cell the K log-likelihoods and posteriors, the best class and, with --class_doublets, the pair
struct ClassScores {
    std::vector<double> ll, post, dpost;
    std::vector<uint8_t> best, call, bpair;
    std::vector<uint64_t> qual;
};
// what class_assignment says of cell c: the best class, or 255 for doublet and 254 for unassigned
// (main.rs:150-153: the doublet call overrides the label, and too few loci override both)
constexpr uint8_t CALL_DOUBLET = 255, CALL_UNASSIGNED = 254;
uint8_t class_call(const Run &run, const ClassScores &s, uint64_t c)
{
    const Params &params = run.params;
    const bool assigned = s.post[(uint64_t)s.best[c] * run.N + c] > params.posterior_threshold && run.entries_per_cell[c] >= params.min_loci_used;
    const bool doublet = params.class_doublets && s.call[c] && run.entries_per_cell[c] >= params.min_loci_used;
    return doublet ? CALL_DOUBLET : assigned ? s.best[c] : CALL_UNASSIGNED;
}

// --refine_classes: one step at a time so that every step gets its stderr line
void refine_classes(const Run &run, const std::vector<std::string> &names, std::vector<uint8_t> &lab, std::vector<uint8_t> &held)
{
    const Ctx &g = run.g;
    const uint32_t K = (uint32_t)names.size();
    for (uint64_t it = 0; it < run.params.refine_classes; it++) {
        cellector_refine_summary rs;
        std::string tail;
        if (run.params.class_doublets) {  // the held-out refine: the called doublets (doublet posterior > 0.5) stay out of every tally
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
        for (uint32_t k = 0; k < K; k++) msg += " " + names[k] + "=" + std::to_string(rs.class_cells[k]);
        msg += tail;
        fprintf(stderr, "%s\n", msg.c_str());
        if (rs.converged) break;
    }
}

// --class_genotypes: a cell counts in the class its class_assignment names; doublet and unassigned cells are in none
void write_class_genotypes(const Run &run, const std::vector<std::string> &names, const ClassScores &s)
{
    const uint64_t N = run.N, TL = run.dims.total_loci;
    const uint32_t K = (uint32_t)names.size();
    std::vector<uint8_t> glab(N);
    for (uint64_t c = 0; c < N; c++) {
        const uint8_t call = class_call(run, s, c);
        glab[c] = call < K ? call : 255;
    }
    // (a run that assigned no cell to any class ends here with the library's refusal: all classes are dead)
    std::vector<uint64_t> galt((uint64_t)(K + 1) * TL), gref((uint64_t)(K + 1) * TL);
    run.g.ck(cellector_class_genotypes(run.g.c, glab.data(), K, VCF_AMBIENT, VCF_GT_THRESHOLD, nullptr, galt.data(), gref.data(), nullptr, nullptr, nullptr),
             "class_genotypes");
    std::vector<uint8_t> gts((uint64_t)K * TL, 0);  // by locus, for the concordance (a locus without a record: no call)
    write_sample_vcf(run, "cellector_classes.vcf",
                     [&](std::string &o) { for (uint32_t k = 0; k < K; k++) { o += '\t'; o += names[k]; } },
                     [&](uint64_t t, std::string &o) {
                         uint64_t A = 0, R = 0;
                         for (uint32_t k = 0; k <= K; k++) { A += galt[(uint64_t)k * TL + t]; R += gref[(uint64_t)k * TL + t]; }
                         const GenotypeLocus gl = genotype_locus(A, R, VCF_AMBIENT);
                         for (uint32_t k = 0; k < K; k++) {
                             const uint64_t a = galt[(uint64_t)k * TL + t], r = gref[(uint64_t)k * TL + t];
                             const GenotypeCall q = genotype_call(gl, a, r, VCF_GT_THRESHOLD);
                             gts[(uint64_t)k * TL + t] = q.gt;
                             put_sample(o, q, a, r);
                         }
                     });
    FILE *fc = create(run.out("cellector_class_concordance.tsv"));
    fputs("class_a\tclass_b\tboth_called\tdiscordant\n", fc);
    for (uint32_t a = 0; a < K; a++)
        for (uint32_t b = a + 1; b < K; b++) {
            uint64_t both = 0, disc = 0;
            for (uint64_t t = 0; t < TL; t++) {
                const uint8_t x = gts[(uint64_t)a * TL + t], y = gts[(uint64_t)b * TL + t];
                both += x && y;
                disc += x && y && x != y;
            }
            fprintf(fc, "%s\t%s\t%llu\t%llu\n", names[a].c_str(), names[b].c_str(), (unsigned long long)both, (unsigned long long)disc);
        }
    fclose(fc);
    run.lap("cellector_classes.vcf");
}

// --classes / --refine_classes: the K-class posteriors of every cell under the file's labelling (or --cluster's), refined if
// asked; then the scoring of the labelling in force, which is returned (--donors names its classes)
ClassLabels run_classes(const Run &run, const ClassLabels &given)
{
    const Params &params = run.params;
    const Ctx &g = run.g;
    const uint64_t N = run.N;
    const CellNames &barcodes = run.in.cells;
    const std::vector<std::string> &names = given.names;
    const uint32_t K = (uint32_t)names.size();
    const std::vector<uint8_t> in_lab(given.label.begin(), given.label.begin() + N);
    std::vector<uint8_t> lab = in_lab;
    const bool dbl = params.class_doublets;
    std::vector<uint8_t> held(dbl ? N : 0, 0);
    refine_classes(run, names, lab, held);
    ClassScores s;
    s.ll.resize((uint64_t)K * N); s.post.resize((uint64_t)K * N); s.qual.resize(N); s.best.resize(N);
    s.dpost.resize(dbl ? N : 0); s.call.resize(dbl ? N : 0); s.bpair.resize(dbl ? 2 * N : 0);
    if (dbl)
        g.ck(cellector_class_doublets(g.c, lab.data(), held.data(), K, nullptr, nullptr, nullptr, nullptr, nullptr, s.ll.data(), nullptr,
                                      s.post.data(), s.dpost.data(), s.best.data(), s.bpair.data(), s.call.data(), s.qual.data()), "class_doublets");
    else
        g.ck(cellector_class_posteriors(g.c, lab.data(), K, nullptr, nullptr, nullptr, s.ll.data(), s.post.data(), s.best.data(), s.qual.data()),
             "class_posteriors");
    std::string head = "barcode\tinput_label\tclass_assignment\tqual";
    for (uint32_t k = 0; k < K; k++) head += "\tlog_likelihood_" + names[k];
    for (uint32_t k = 0; k < K; k++) head += "\tposterior_" + names[k];
    if (dbl) head += "\tdoublet_posterior\tdoublet_pair";
    head += '\n';
    write_tsv(run.out("cellector_classes.tsv"), head, N, [&](uint64_t c, std::string &o) {
        const uint8_t call = class_call(run, s, c);
        o += barcodes[c]; o += '\t'; o += in_lab[c] == 255 ? "na" : names[in_lab[c]].c_str(); o += '\t';
        o += call == CALL_DOUBLET ? "doublet" : call == CALL_UNASSIGNED ? "unassigned" : names[call].c_str(); o += '\t'; put(o, s.qual[c]);
        for (uint32_t k = 0; k < K; k++) { o += '\t'; put(o, s.ll[(uint64_t)k * N + c]); }
        for (uint32_t k = 0; k < K; k++) { o += '\t'; put(o, s.post[(uint64_t)k * N + c]); }
        if (dbl) {
            o += '\t'; put(o, s.dpost[c]); o += '\t';
            if (s.bpair[2 * c] == 255) o += "na";
            else { o += names[s.bpair[2 * c]]; o += '+'; o += names[s.bpair[2 * c + 1]]; }
        }
        o += '\n';
    });
    run.lap("cellector_classes.tsv");
    if (params.class_genotypes) write_class_genotypes(run, names, s);
    return {lab, names};
}

// ---- --donors -----------------------------------------------------------------------------------------------------------
const char *donor_status(uint8_t status)
{
    static const char *const STATUS[3] = {"singlet", "doublet", "ambiguous"};
    return status < 3 ? STATUS[status] : "unassigned";
}

// the donors' genotypes and the parameters of their passes
struct Donors {
    DonorGenotypes dg;
    bool soft = false;             // --donor_field GP / GL / PL: the soft calls score the weights ...
    std::vector<uint8_t> hard_gt;  // ... and what needs a hard call takes every row's most probable genotype
    uint32_t D = 0;
    cellector_donor_params dp;
    const uint8_t *gt_codes() const { return soft ? hard_gt.data() : dg.gt.data(); }
    const std::string &name(uint32_t d) const { return dg.names[d]; }
};
// --donor_field: call(entry point, the donors' calls as that entry takes them, its name) with the hard pair or the soft one
template <class Hard, class Soft, class F>
void with_donor_calls(const Donors &d, Hard hard, const char *hard_name, Soft soft, const char *soft_name, F call)
{
    if (d.soft) call(soft, d.dg.gp.data(), soft_name);
    else call(hard, d.dg.gt.data(), hard_name);
}

Donors read_donors(const Run &run)
{
    const Params &params = run.params;
    Donors d;
    d.soft = params.donor_field != "GT";
    if (d.soft) d.dg.field = params.donor_field;
    {
        Lines vin(*params.vcf);
        std::string line;
        while (vin.next(line)) d.dg.add_variant_line(line);
        Lines din(*params.donors);
        while (din.next(line)) d.dg.add_donor_line(line);
    }
    d.D = (uint32_t)d.dg.names.size();
    if (params.donor_panel && (d.D < 1 || d.D > 4096))
        die(1, "error: --donors " + *params.donors + ": " + std::to_string(d.dg.names.size()) + " sample columns, --donor_panel takes 1..4096 donors");
    if (!params.donor_panel && (d.D < 1 || d.D > 64))
        die(1, "error: --donors " + *params.donors + ": " + std::to_string(d.dg.names.size()) + " sample columns, 1..64 donors are supported");
    if (d.dg.total_loci != run.dims.total_loci)
        die(1, "error: --donors: --vcf " + *params.vcf + " has " + std::to_string(d.dg.total_loci) + " records but the matrix has " +
                   std::to_string(run.dims.total_loci) + " loci");
    cellector_donor_default_params(&d.dp);
    d.dp.err = params.donor_error; d.dp.ambient = params.donor_ambient; d.dp.doublet_rate = params.donor_doublet_rate;
    d.dp.posterior_threshold = params.posterior_threshold;
    d.dp.min_loci = std::max<uint64_t>(params.min_loci_used, 1);
    if (d.soft) d.hard_gt = donor_hard_codes(d.dg.gp);
    return d;
}

struct DonorCalls {
    std::vector<double> ll, post, ppost, dbl;
    std::vector<uint8_t> best, second, pair, status;
    std::vector<uint32_t> n;
};
DonorCalls donor_pass(const Run &run, const Donors &d)
{
    const uint64_t N = run.N, ND = N * d.D;
    DonorCalls r{std::vector<double>(ND), std::vector<double>(ND), std::vector<double>(ND), std::vector<double>(N), std::vector<uint8_t>(N),
                 std::vector<uint8_t>(N),  std::vector<uint8_t>(N),  std::vector<uint8_t>(N),  std::vector<uint32_t>(N)};
    cellector_donor_summary ds;
    with_donor_calls(d, cellector_donor_posteriors, "donor_posteriors", cellector_donor_posteriors_gp, "donor_posteriors_gp",
                     [&](auto entry, auto *calls, const char *what) {
                         run.g.ck(entry(run.g.c, calls, d.D, &d.dp, nullptr, nullptr, nullptr, r.ll.data(), nullptr, r.post.data(), r.ppost.data(),
                                        r.dbl.data(), r.best.data(), r.second.data(), r.pair.data(), r.n.data(), r.status.data(), nullptr, &ds,
                                        nullptr, nullptr), what);
                     });
    fprintf(stderr, "donors: %u donors, singlet=%llu doublet=%llu ambiguous=%llu unassigned=%llu\n", d.D,
            (unsigned long long)ds.n_singlet, (unsigned long long)ds.n_doublet, (unsigned long long)ds.n_ambiguous,
            (unsigned long long)ds.n_unassigned);
    return r;
}

// --estimate_ambient: the pool's ambient fraction from the singlets, each under its best donor; returns the pooled estimate
double write_ambient(const Run &run, const Donors &d, const DonorCalls &calls)
{
    const uint64_t N = run.N;
    const CellNames &barcodes = run.in.cells;
    std::vector<uint8_t> assign(N);
    for (uint64_t c = 0; c < N; c++) assign[c] = calls.status[c] == 0 ? calls.best[c] : (uint8_t)255;
    cellector_ambient_params ap;
    cellector_ambient_default_params(&ap);
    ap.err = run.params.donor_error;
    cellector_ambient_summary as;
    std::vector<double> crho(N), cse(N);
    std::vector<uint32_t> cn(N);
    run.g.ck(cellector_estimate_ambient(run.g.c, d.gt_codes(), d.D, assign.data(), &ap, nullptr, &as, crho.data(), cse.data(), cn.data()),
             "estimate_ambient");
    {
        std::string o = "ambient: rho=";
        put(o, as.rho); o += " se="; put(o, as.se); o += " cells="; put(o, as.n_cells_used);
        o += as.at_boundary ? " at_boundary=1\n" : " at_boundary=0\n";
        fputs(o.c_str(), stdout);
    }
    FILE *fa = create(run.out("cellector_ambient.tsv"));
    fputs("source\tcells\trho\tse\n", fa);
    {
        std::string o = "pool\t";
        put(o, as.n_cells_used); o += '\t'; put(o, as.rho); o += '\t'; put(o, as.se); o += '\n';
        for (uint32_t k = 0; k < d.D; k++) {
            o += d.name(k); o += '\t'; put(o, as.source_cells[k]); o += '\t';
            if (as.source_cells[k]) { put(o, as.source_rho[k]); o += '\t'; put(o, as.source_se[k]); }
            else o += "NA\tNA";
            o += '\n';
        }
        fputs(o.c_str(), fa);
    }
    fclose(fa);
    write_tsv(run.out("cellector_ambient_cells.tsv"), "barcode\tdonor\tn_loci\trho\tse\n", N, [&](uint64_t c, std::string &o) {
        o += barcodes[c]; o += '\t';
        if (assign[c] == 255) { o += "NA\tNA\tNA\tNA\n"; return; }
        o += d.name(assign[c]); o += '\t'; put(o, (uint64_t)cn[c]); o += '\t';
        if (crho[c] != crho[c]) o += "NA\tNA";
        else { put(o, crho[c]); o += '\t'; put(o, cse[c]); }
        o += '\n';
    });
    run.lap("cellector_ambient.tsv");
    return as.rho;
}

void write_donors_tsv(const Run &run, const Donors &d, const DonorCalls &r)
{
    const uint32_t D = d.D;
    const CellNames &barcodes = run.in.cells;
    std::string head = "barcode\tstatus\tdonor\tsecond_donor\tbest_pair\tposterior\tpair_posterior\tdoublet_posterior\tn_loci";
    for (uint32_t k = 0; k < D; k++) head += "\tlog_likelihood_" + d.name(k);
    head += '\n';
    write_tsv(run.out("cellector_donors.tsv"), head, run.N, [&](uint64_t c, std::string &o) {
        const uint8_t b = r.best[c];
        o += barcodes[c]; o += '\t'; o += donor_status(r.status[c]); o += '\t';
        o += d.name(b); o += '\t';
        o += r.second[c] == 255 ? "na" : d.name(r.second[c]).c_str(); o += '\t';
        if (r.pair[c] == 255) o += "na";
        else { o += d.name(b); o += '+'; o += d.name(r.pair[c]); }
        o += '\t'; put(o, r.post[c * D + b]);
        o += '\t'; put(o, r.pair[c] == 255 ? 0.0 : r.ppost[c * D + r.pair[c]]);
        o += '\t'; put(o, r.dbl[c]);
        o += '\t'; put(o, (uint64_t)r.n[c]);
        for (uint32_t k = 0; k < D; k++) { o += '\t'; put(o, r.ll[c * D + k]); }
        o += '\n';
    });
    run.lap("cellector_donors.tsv");
}

// --donor_fit: the fit of the called hypothesis under the hard calls and the parameters the donor pass ended with
void write_donor_fit(const Run &run, const Donors &d)
{
    const Ctx &g = run.g;
    const uint64_t N = run.N, ND = N * d.D;
    const uint32_t D = d.D;
    const CellNames &barcodes = run.in.cells;
    cellector_donor_fit_params fp;
    cellector_donor_fit_default_params(&fp);
    if (run.params.donor_fit_iqr) fp.iqr_multiple = *run.params.donor_fit_iqr;
    std::vector<double> fe(ND), fv(ND), fpe(ND), fpv(ND), fll(ND), fpll(ND), fz(N);
    std::vector<uint8_t> ha(N), hb(N), fstatus(N), unmatched(N);
    std::vector<uint32_t> fn(N);
    cellector_donor_fit_summary fs;
    g.ck(cellector_donor_fit(g.c, d.gt_codes(), D, &d.dp, &fp, nullptr, nullptr, nullptr, fe.data(), fv.data(), fpe.data(), fpv.data(), nullptr,
                             nullptr, fz.data(), ha.data(), hb.data(), fstatus.data(), unmatched.data(), &fs, nullptr, nullptr),
         "donor_fit");
    // the sums of the called hypothesis: the hard call's own ll and pair_ll (the bits the fit took its z from)
    g.ck(cellector_donor_posteriors(g.c, d.gt_codes(), D, &d.dp, nullptr, nullptr, nullptr, fll.data(), fpll.data(), nullptr, nullptr, nullptr,
                                    nullptr, nullptr, nullptr, fn.data(), nullptr, nullptr, nullptr, nullptr, nullptr),
         "donor_posteriors");
    {
        std::string o = "donor_fit: keys=";
        put(o, fs.n_keys); o += " median="; put(o, fs.median); o += " iqr="; put(o, fs.iqr); o += " threshold="; put(o, fs.threshold);
        o += " unmatched="; put(o, fs.n_unmatched); o += '\n';
        fputs(o.c_str(), stdout);
    }
    write_tsv(run.out("cellector_donor_fit.tsv"), "barcode\tstatus\tdonor\tsecond_donor\tn_loci\tll\texpected\tvariance\tz\tunmatched\n", N,
              [&](uint64_t c, std::string &o) {
                  o += barcodes[c]; o += '\t'; o += donor_status(fstatus[c]); o += '\t';
                  if (fstatus[c] == 255) {
                      o += "NA\tNA\t"; put(o, (uint64_t)fn[c]); o += "\tNA\tNA\tNA\tNA\tNA\n";
                      return;
                  }
                  const bool pair = hb[c] != 255;
                  const uint64_t at = c * D + (pair ? hb[c] : ha[c]);
                  o += d.name(ha[c]); o += '\t'; o += pair ? d.name(hb[c]).c_str() : "NA"; o += '\t'; put(o, (uint64_t)fn[c]);
                  o += '\t'; put(o, pair ? fpll[at] : fll[at]);
                  o += '\t'; put(o, pair ? fpe[at] : fe[at]);
                  o += '\t'; put(o, pair ? fpv[at] : fv[at]);
                  o += '\t'; put(o, fz[c]);
                  o += unmatched[c] ? "\t1\n" : "\t0\n";
              });
    run.lap("cellector_donor_fit.tsv");
}

// --doublet_fraction: the mixing share of every called doublet under (the donor pass' anchor, its best pair), the hard calls and the
// parameters the donor pass ended with
void write_doublet_fractions(const Run &run, const Donors &d, const DonorCalls &calls)
{
    static const char *const KIND[4] = {"balanced", "toward_a", "toward_b", "flat"};
    const uint64_t N = run.N, G = 17;
    const CellNames &barcodes = run.in.cells;
    std::vector<uint8_t> pa(N), pb(N);
    for (uint64_t c = 0; c < N; c++) {
        const bool dbl = calls.status[c] == 1 && calls.pair[c] != 255;
        pa[c] = dbl ? calls.best[c] : (uint8_t)255;  // (no anchor was given: the pass anchored every cell at its best donor)
        pb[c] = dbl ? calls.pair[c] : (uint8_t)255;
    }
    cellector_pair_fraction_params fp;
    cellector_pair_fraction_default_params(&fp);
    if (run.params.doublet_min_fraction) fp.min_fraction = *run.params.doublet_min_fraction;
    fp.min_loci = d.dp.min_loci;
    std::vector<double> ll(N * G), frac(N), se(N);
    std::vector<uint32_t> cn(N);
    std::vector<uint8_t> js(N), kind(N);
    cellector_pair_fraction_summary fs;
    run.g.ck(cellector_donor_pair_fractions(run.g.c, d.gt_codes(), d.D, &d.dp, &fp, pa.data(), pb.data(), nullptr, 0, nullptr, ll.data(),
                                            cn.data(), frac.data(), se.data(), js.data(), kind.data(), &fs, nullptr),
             "donor_pair_fractions");
    {
        std::string o = "doublet_fraction: balanced=";
        put(o, fs.n_balanced); o += " toward_a="; put(o, fs.n_toward_a); o += " toward_b="; put(o, fs.n_toward_b);
        o += " flat="; put(o, fs.n_flat); o += " none="; put(o, fs.n_none); o += '\n';
        fputs(o.c_str(), stdout);
    }
    write_tsv(run.out("cellector_doublet_fractions.tsv"), "barcode\tdonor_a\tdonor_b\tn_loci\tfraction\tse\tll_half\tll_max\tkind\n", N,
              [&](uint64_t c, std::string &o) {
                  o += barcodes[c];
                  if (pa[c] == 255) { o += "\tNA\tNA\tNA\tNA\tNA\tNA\tNA\tNA\n"; return; }
                  o += '\t'; o += d.name(pa[c]); o += '\t'; o += d.name(pb[c]); o += '\t'; put(o, (uint64_t)cn[c]); o += '\t';
                  if (kind[c] == 255) o += "NA\tNA";
                  else { put(o, frac[c]); o += '\t'; put(o, se[c]); }
                  o += '\t'; put(o, ll[c * G + G / 2]); o += '\t'; put(o, ll[c * G + js[c]]); o += '\t';
                  o += kind[c] < 4 ? KIND[kind[c]] : "NA"; o += '\n';
              });
    run.lap("cellector_doublet_fractions.tsv");
}

// --donor_genotypes: the donors' genotypes from the reads of the status-0 cells, each under its best donor, with the donors' own
// rows as the prior (--donor_field GT: the one-hot of the hard calls) and the parameters the donor pass ended with.  Returns q as
// the float rows cellector_donor_posteriors_gp takes (apply scores the donors again with them).
std::vector<float> write_donor_genotypes(const Run &run, const Donors &d, const DonorCalls &calls)
{
    const uint64_t N = run.N, TL = run.dims.total_loci;
    const uint32_t D = d.D;
    std::vector<uint8_t> assign(N);
    for (uint64_t c = 0; c < N; c++) assign[c] = calls.status[c] == 0 ? calls.best[c] : (uint8_t)255;
    std::vector<float> prior;
    if (d.soft) {
        prior = d.dg.gp;
    } else {
        prior.assign((uint64_t)D * TL * 3, 0.f);
        for (uint64_t i = 0; i < (uint64_t)D * TL; i++) {
            const uint8_t g = d.dg.gt[i];
            if (g < 3) prior[3 * i + g] = 1.f;
            else prior[3 * i] = prior[3 * i + 1] = prior[3 * i + 2] = std::numeric_limits<float>::quiet_NaN();
        }
    }
    cellector_donor_genotypes_params gp;
    cellector_donor_genotypes_default_params(&gp);
    gp.err = d.dp.err; gp.ambient = d.dp.ambient;
    std::vector<uint64_t> galt((uint64_t)(D + 1) * TL), gref((uint64_t)(D + 1) * TL);
    std::vector<double> q((uint64_t)D * TL * 3);
    std::vector<uint8_t> gt((uint64_t)D * TL);
    cellector_donor_genotypes_summary gs;
    run.g.ck(cellector_donor_genotypes(run.g.c, assign.data(), prior.data(), D, &gp, nullptr, galt.data(), gref.data(), q.data(), gt.data(), nullptr,
                                       &gs, nullptr, nullptr), "donor_genotypes");
    {
        uint64_t tot[5] = {};
        for (uint32_t k = 0; k < D; k++) {
            tot[0] += gs.cells[k]; tot[1] += gs.confirmed[k]; tot[2] += gs.filled[k]; tot[3] += gs.changed[k]; tot[4] += gs.withdrawn[k];
        }
        std::string o = "donor_genotypes: donors=";
        put(o, (uint64_t)D); o += " cells="; put(o, tot[0]); o += " confirmed="; put(o, tot[1]); o += " filled="; put(o, tot[2]);
        o += " changed="; put(o, tot[3]); o += " withdrawn="; put(o, tot[4]); o += '\n';
        fputs(o.c_str(), stdout);
    }
    static const char *const GT[4] = {"0/0", "0/1", "1/1", "./."};
    write_sample_vcf(run, "cellector_donor_genotypes.vcf",
                     [&](std::string &o) { for (uint32_t k = 0; k < D; k++) { o += '\t'; o += d.name((uint8_t)k); } },
                     [&](uint64_t t, std::string &o) {
                         for (uint32_t k = 0; k < D; k++) {
                             const uint64_t i = (uint64_t)k * TL + t;
                             o += '\t'; o += GT[gt[i] & 3]; o += ':';
                             put(o, q[3 * i]); o += ','; put(o, q[3 * i + 1]); o += ','; put(o, q[3 * i + 2]); o += ':';
                             put(o, galt[i]); o += ':'; put(o, gref[i]);
                         }
                     });
    FILE *f = create(run.out("cellector_donor_genotypes.tsv"));
    {
        std::string o = "donor\tcells\tloci_with_reads\tconfirmed\tfilled\tchanged\twithdrawn\n";
        for (uint32_t k = 0; k < D; k++) {
            o += d.name((uint8_t)k);
            for (const uint64_t v : {gs.cells[k], gs.loci_with_reads[k], gs.confirmed[k], gs.filled[k], gs.changed[k], gs.withdrawn[k]}) {
                o += '\t'; put(o, v);
            }
            o += '\n';
        }
        fputs(o.c_str(), f);
    }
    fclose(f);
    run.lap("cellector_donor_genotypes.vcf");
    return std::vector<float>(q.begin(), q.end());
}

// the classes in force named by donor
void write_cluster_donors(const Run &run, const Donors &d, const ClassLabels &classes)
{
    const uint32_t K = (uint32_t)classes.names.size(), D = d.D;
    std::vector<uint8_t> lab(classes.label.begin(), classes.label.begin() + run.N), mbest(K);
    std::vector<double> mll((uint64_t)K * D), margin(K);
    std::vector<uint64_t> mcells(K);
    with_donor_calls(d, cellector_match_donors, "match_donors", cellector_match_donors_gp, "match_donors_gp",
                     [&](auto entry, auto *calls, const char *what) {
                         run.g.ck(entry(run.g.c, lab.data(), K, calls, D, &d.dp, nullptr, mll.data(), mbest.data(), margin.data(), mcells.data()), what);
                     });
    FILE *fm = create(run.out("cellector_cluster_donors.tsv"));
    std::string mh = "class\tcells\tdonor\tmargin";
    for (uint32_t k = 0; k < D; k++) mh += "\tlog_likelihood_" + d.name(k);
    mh += '\n';
    fputs(mh.c_str(), fm);
    for (uint32_t k = 0; k < K; k++) {
        std::string o = classes.names[k];
        o += '\t'; put(o, mcells[k]); o += '\t'; o += mbest[k] == 255 ? "na" : d.name(mbest[k]).c_str(); o += '\t'; put(o, margin[k]);
        for (uint32_t j = 0; j < D; j++) { o += '\t'; put(o, mll[(uint64_t)k * D + j]); }
        o += '\n';
        fputs(o.c_str(), fm);
    }
    fclose(fm);
    run.lap("cellector_cluster_donors.tsv");
}

// --donor_panel: every cell against the whole panel (cellector_donor_panel), the panel's two files and, with classes in force, the
// classes named by panel donor.  The donors with --donor_panel_min_cells status-0 cells replace the panel in d, in panel order; false
// where the donor pass cannot follow (none or more than 64 present).
bool run_donor_panel(const Run &run, Donors &d, const ClassLabels &classes)
{
    const Params &params = run.params;
    const uint64_t N = run.N, TL = run.dims.total_loci;
    const uint32_t D = d.D, asked = (uint32_t)params.donor_panel, M = std::min(asked, D);
    const CellNames &barcodes = run.in.cells;
    std::vector<uint16_t> cand(N * M), best(N), second(N), pair(N), anchor(N);
    std::vector<double> cll(N * M), cpost(N * M), cppost(N * M), dbl(N), bpost(N);
    std::vector<uint32_t> n(N);
    std::vector<uint8_t> status(N);
    std::vector<uint64_t> cells(D), dcells(D, 0);
    cellector_donor_panel_summary ps;
    run.g.ck(cellector_donor_panel(run.g.c, d.dg.gt.data(), D, asked, &d.dp, nullptr, nullptr, nullptr, cand.data(), cll.data(), nullptr,
                                   cpost.data(), cppost.data(), dbl.data(), bpost.data(), best.data(), second.data(), pair.data(),
                                   anchor.data(), n.data(), status.data(), cells.data(), &ps, nullptr, nullptr, nullptr, nullptr),
             "donor_panel");
    uint64_t n_present = 0;
    for (uint32_t k = 0; k < D; k++) n_present += cells[k] >= params.donor_panel_min_cells;
    fprintf(stderr, "donor_panel: %u donors, shortlist %u, singlet=%llu doublet=%llu ambiguous=%llu unassigned=%llu present=%llu\n", D, asked,
            (unsigned long long)ps.n_singlet, (unsigned long long)ps.n_doublet, (unsigned long long)ps.n_ambiguous,
            (unsigned long long)ps.n_unassigned, (unsigned long long)n_present);
    std::string head = "barcode\tstatus\tdonor\tsecond_donor\tbest_pair\tposterior\tpair_posterior\tdoublet_posterior\tn_loci";
    for (uint32_t j = 0; j < asked; j++) {
        const std::string t = std::to_string(j);
        head += "\tcandidate_" + t + "\tlog_likelihood_" + t + "\tposterior_" + t;
    }
    head += '\n';
    write_tsv(run.out("cellector_donor_panel.tsv"), head, N, [&](uint64_t c, std::string &o) {
        o += barcodes[c]; o += '\t'; o += donor_status(status[c]); o += '\t';
        o += d.name(best[c]); o += '\t';
        o += second[c] == 65535 ? "NA" : d.name(second[c]).c_str(); o += '\t';
        double pp = 0.0;
        if (pair[c] == 65535) o += "NA";
        else {
            o += d.name(anchor[c]); o += '+'; o += d.name(pair[c]);
            for (uint32_t j = 0; j < M; j++)
                if (cand[c * M + j] == pair[c]) pp = cppost[c * M + j];
        }
        o += '\t'; put(o, bpost[c]);
        o += '\t'; put(o, pp);
        o += '\t'; put(o, dbl[c]);
        o += '\t'; put(o, (uint64_t)n[c]);
        for (uint32_t j = 0; j < asked; j++) {
            if (j >= M) { o += "\tNA\tNA\tNA"; continue; }
            o += '\t'; o += d.name(cand[c * M + j]); o += '\t'; put(o, cll[c * M + j]); o += '\t'; put(o, cpost[c * M + j]);
        }
        o += '\n';
    });
    for (uint64_t c = 0; c < N; c++)
        if (status[c] == 1 && pair[c] != 65535) { dcells[anchor[c]]++; dcells[pair[c]]++; }
    {
        FILE *f = create(run.out("cellector_donor_panel_donors.tsv"));
        std::string o = "donor\tsinglet_cells\tdoublet_cells\tpresent\n";
        for (uint32_t k = 0; k < D; k++) {
            o += d.name(k); o += '\t'; put(o, cells[k]); o += '\t'; put(o, dcells[k]);
            o += cells[k] >= params.donor_panel_min_cells ? "\t1\n" : "\t0\n";
        }
        fputs(o.c_str(), f);
        fclose(f);
    }
    run.lap("cellector_donor_panel.tsv");
    if (params.classes || params.cluster) {
        const uint32_t K = (uint32_t)classes.names.size();
        std::vector<uint8_t> lab(classes.label.begin(), classes.label.begin() + N);
        std::vector<uint16_t> mbest(K);
        std::vector<double> margin(K);
        std::vector<uint64_t> mcells(K);
        run.g.ck(cellector_match_donors_panel(run.g.c, lab.data(), K, d.dg.gt.data(), D, &d.dp, nullptr, nullptr, mbest.data(), margin.data(),
                                              mcells.data()), "match_donors_panel");
        FILE *fm = create(run.out("cellector_cluster_panel_donors.tsv"));
        std::string o = "class\tcells\tdonor\tmargin\n";
        for (uint32_t k = 0; k < K; k++) {
            o += classes.names[k]; o += '\t'; put(o, mcells[k]); o += '\t'; o += mbest[k] == 65535 ? "NA" : d.name(mbest[k]).c_str();
            o += '\t'; put(o, margin[k]); o += '\n';
        }
        fputs(o.c_str(), fm);
        fclose(fm);
        run.lap("cellector_cluster_panel_donors.tsv");
    }
    if (n_present < 1 || n_present > 64) {
        fprintf(stderr, "donor_panel: %llu donors are present, the donor pass takes 1..64: skipped\n", (unsigned long long)n_present);
        if (params.estimate_ambient || params.donor_fit || params.doublet_fraction || params.donor_genotypes)
            die(1, "error: --donor_panel found " + std::to_string(n_present) + " donors present; --estimate_ambient, --donor_fit, "
                   "--doublet_fraction and --donor_genotypes need the donor pass over 1..64 of them");
        return false;
    }
    // the present donors, in panel order, as if the VCF held only their columns
    std::vector<std::string> names;
    std::vector<uint8_t> gt;
    for (uint32_t k = 0; k < D; k++) {
        if (cells[k] < params.donor_panel_min_cells) continue;
        names.push_back(d.dg.names[k]);
        gt.insert(gt.end(), d.dg.gt.begin() + (uint64_t)k * TL, d.dg.gt.begin() + (uint64_t)(k + 1) * TL);
    }
    d.dg.names = std::move(names);
    d.dg.gt = std::move(gt);
    d.D = (uint32_t)n_present;
    return true;
}

// --donors: every cell against the genotyped donors of the pool, and the classes in force (--classes / --cluster, refined if asked)
// named by donor
void run_donors(const Run &run, const ClassLabels &classes)
{
    const Params &params = run.params;
    Donors d = read_donors(run);
    if (params.donor_panel && !run_donor_panel(run, d, classes)) return;
    DonorCalls calls = donor_pass(run, d);
    if (params.estimate_ambient) {
        const double rho = write_ambient(run, d, calls);
        if (params.estimate_ambient == 2) {  // apply: the donors again with it
            d.dp.ambient = rho;
            calls = donor_pass(run, d);
        }
    }
    if (params.donor_genotypes) {
        std::vector<float> refined = write_donor_genotypes(run, d, calls);
        if (params.donor_genotypes == 2) {  // apply: the donors again, under the refined rows as genotype weights
            d.soft = true;
            d.dg.gp = std::move(refined);
            d.hard_gt = donor_hard_codes(d.dg.gp);
            calls = donor_pass(run, d);
        }
    }
    write_donors_tsv(run, d, calls);
    if (params.donor_fit) write_donor_fit(run, d);
    if (params.doublet_fraction) write_doublet_fractions(run, d, calls);
    if (params.classes || params.cluster) write_cluster_donors(run, d, classes);
}

}  // namespace

int main(int argc, char **argv)
{
    const Params params = load_params(argc, argv);
    Run run(params, read_inputs(params));
    run.g = open_device(params, run.devices);
    run.lap("barcodes + device init");
    load_matrix(run);
    if (params.initial_minority) set_initial_minority(run);
    if (params.vcf) run.vcf_data = load_vcf_data(*params.vcf);

    const LoopResult loop = run_loop(run);
    run.lap("EM loop + iteration files");
    const Posteriors posteriors = run_posteriors(run);
    run.lap("posteriors");
    if (params.vcf) write_final_vcf(run);
    run.lap("final tallies + cellector.vcf");
    if (params.cell_detail) write_cell_detail(run);
    const ConfusionCounts counts = write_assignments(run, loop, posteriors);
    run.lap("assignments file");
    print_confusion_table(counts);

    ClassLabels classes = run.in.classes;
    if (params.cluster) classes = run_cluster(run);
    if (params.classes || (params.cluster && (params.refine_classes || params.class_doublets || params.class_genotypes)))
        classes = run_classes(run, classes);
    if (params.donors) run_donors(run, classes);

    // Every output file is closed: leave without tearing the context down.  Handing ~150 GB of device memory back block
    // by block (and destroying the host vectors) was half a second of the 1M x 200k run; the driver reclaims a dead
    // process' memory in one go.
    fflush(stdout);
    fflush(stderr);
    // (a multi-device ctx always leaves the orderly way: its communicator and worker threads are torn down in order;
    //  so does a run under a profiler or leak checker, CELLECTOR_TEARDOWN=1)
    if (run.devices.size() > 1 || getenv("CELLECTOR_TEARDOWN")) {
        cellector_destroy(run.g.c);
        return 0;
    }
    _exit(0);
}
