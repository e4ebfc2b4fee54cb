// The donors' genotypes from a VCF, for the CLI's --donors (host/cellector.cpp) and its CPU test: plain C++, no device code, no I/O of
// its own (the caller feeds it lines).  The rule is cellector_amd/donors.py's read_donor_vcf: a donor record is matched to the variant
// VCF's record with the same (chrom, pos, ref, alt); one whose ref and alt are swapped is matched too and its calls are mirrored; a
// variant without a donor record, and a missing, unparsable or non-biallelic GT, is 3 (no call); of repeated records the last counts.
#pragma once
#include <cstdint>
#include <map>
#include <string>
#include <string_view>
#include <vector>

constexpr uint8_t DONOR_NO_CALL = 3;

inline std::vector<std::string_view> donor_split(std::string_view s, char sep)
{
    std::vector<std::string_view> out;
    size_t b = 0;
    for (;;) {
        const size_t e = s.find(sep, b);
        if (e == std::string_view::npos) { out.push_back(s.substr(b)); return out; }
        out.push_back(s.substr(b, e - b));
        b = e + 1;
    }
}

// 0, 1 or 2 = the alt alleles of a diploid biallelic GT ("0/1", "1|0", ...) at position gt_index of a sample field; 3 otherwise
inline uint8_t donor_parse_gt(std::string_view field, int gt_index)
{
    const std::vector<std::string_view> parts = donor_split(field, ':');
    if (gt_index < 0 || (size_t)gt_index >= parts.size()) return DONOR_NO_CALL;
    const std::string_view g = parts[(size_t)gt_index];
    if (g.size() != 3 || (g[1] != '/' && g[1] != '|')) return DONOR_NO_CALL;
    if ((g[0] != '0' && g[0] != '1') || (g[2] != '0' && g[2] != '1')) return DONOR_NO_CALL;
    return (uint8_t)((g[0] - '0') + (g[2] - '0'));
}

struct DonorGenotypes {
    std::vector<std::string> names;  // [D] the sample columns of the donor VCF's #CHROM line
    std::vector<uint8_t> gt;         // [D][total_loci], made (all 3) at that line, filled by the records behind it
    uint64_t total_loci = 0;

    // every line of the variant VCF, in file order (header lines are skipped)
    void add_variant_line(std::string_view line)
    {
        if (line.empty() || line[0] == '#') return;
        const std::vector<std::string_view> t = donor_split(line, '\t');
        if (t.size() >= 5) rows_[key(t[0], t[1], t[3], t[4])] = total_loci;
        total_loci++;
    }
    // every line of the donor VCF, after all variant lines
    void add_donor_line(std::string_view line)
    {
        if (line.empty()) return;
        if (line[0] == '#') {
            if (line.rfind("#CHROM", 0) == 0) {
                const std::vector<std::string_view> t = donor_split(line, '\t');
                names.clear();
                for (size_t i = 9; i < t.size(); i++) names.emplace_back(t[i]);
                gt.assign(names.size() * total_loci, DONOR_NO_CALL);
            }
            return;
        }
        const std::vector<std::string_view> t = donor_split(line, '\t');
        if (t.size() < 10) return;
        bool swap = false;
        auto at = rows_.find(key(t[0], t[1], t[3], t[4]));
        if (at == rows_.end()) { at = rows_.find(key(t[0], t[1], t[4], t[3])); swap = true; }
        if (at == rows_.end()) return;
        const std::vector<std::string_view> fmt = donor_split(t[8], ':');
        int gi = -1;
        for (size_t i = 0; i < fmt.size(); i++)
            if (fmt[i] == "GT") { gi = (int)i; break; }
        for (size_t d = 0; d < names.size(); d++) {
            const uint8_t g = 9 + d < t.size() ? donor_parse_gt(t[9 + d], gi) : DONOR_NO_CALL;
            gt[d * total_loci + at->second] = g == DONOR_NO_CALL || !swap ? g : (uint8_t)(2 - g);
        }
    }

private:
    static std::string key(std::string_view chrom, std::string_view pos, std::string_view ref, std::string_view alt)
    {
        std::string k(chrom);
        k += '\t'; k += pos; k += '\t'; k += ref; k += '\t'; k += alt;
        return k;
    }
    std::map<std::string, uint64_t> rows_;
};
