// The donors' genotypes from a VCF, for the CLI's --donors (host/cellector.cpp) and its CPU test: plain C++, no device code, no I/O of
// its own (the caller feeds it lines).  The rule is cellector_amd/donors.py's read_donor_vcf: a donor record is matched to the variant
// VCF's record with the same (chrom, pos, ref, alt); one whose ref and alt are swapped is matched too and its calls are mirrored; a
// variant without a donor record, and a missing, unparsable or non-biallelic GT, is 3 (no call); of repeated records the last counts.
// With a field (GP, GL or PL; --donor_field) the three weights of every sample are read beside its GT, by read_donor_vcf_gp's rule.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <limits>
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

// a plain decimal number, [+-]digits[.digits][e[+-]digits] or [+-].digits[e...], and nothing else (no nan, no inf, no hex)
inline bool donor_parse_number(std::string_view s, double *out)
{
    size_t i = 0, digits = 0;
    const auto run = [&]() { size_t n = 0; while (i < s.size() && s[i] >= '0' && s[i] <= '9') { i++; n++; } return n; };
    if (i < s.size() && (s[i] == '+' || s[i] == '-')) i++;
    digits = run();
    if (i < s.size() && s[i] == '.') { i++; const size_t frac = run(); if (!digits && !frac) return false; digits += frac; }
    if (!digits) return false;
    if (i < s.size() && (s[i] == 'e' || s[i] == 'E')) {
        i++;
        if (i < s.size() && (s[i] == '+' || s[i] == '-')) i++;
        if (!run()) return false;
    }
    if (i != s.size()) return false;
    *out = strtod(std::string(s).c_str(), nullptr);
    return true;
}

// The three weights of a sample field's GP ('P'), GL ('L') or PL ('Q') at position index, in double; false: the field absent, ".",
// not three plain numbers, a GP or PL below 0, a value that is not finite, or three zeros.  GP: as written.  GL: 10^(GL_g - max GL).
// PL: 10^(-(PL_g - min PL) / 10).
inline bool donor_parse_weights(std::string_view field, int index, char kind, double out[3])
{
    const std::vector<std::string_view> parts = donor_split(field, ':');
    if (index < 0 || (size_t)index >= parts.size()) return false;
    const std::vector<std::string_view> toks = donor_split(parts[(size_t)index], ',');
    if (toks.size() != 3) return false;
    double v[3];
    for (int g = 0; g < 3; g++)
        if (!donor_parse_number(toks[(size_t)g], &v[g]) || !std::isfinite(v[g]) || (kind != 'L' && v[g] < 0)) return false;
    const double hi = std::fmax(v[0], std::fmax(v[1], v[2])), lo = std::fmin(v[0], std::fmin(v[1], v[2]));
    for (int g = 0; g < 3; g++) v[g] = kind == 'L' ? std::pow(10.0, v[g] - hi) : kind == 'Q' ? std::pow(10.0, -(v[g] - lo) / 10.0) : v[g];
    if (!(v[0] > 0 || v[1] > 0 || v[2] > 0)) return false;
    for (int g = 0; g < 3; g++) out[g] = v[g];  // (out is written only when the weights count)
    return true;
}

// gt [rows] from gp [rows][3]: the argmax of every row, the smallest g on ties, 3 for a no-call (three NaN)
inline std::vector<uint8_t> donor_hard_codes(const std::vector<float> &gp)
{
    std::vector<uint8_t> out(gp.size() / 3, DONOR_NO_CALL);
    for (size_t i = 0; i < out.size(); i++) {
        const float *r = gp.data() + 3 * i;
        if (std::isnan(r[0]) && std::isnan(r[1]) && std::isnan(r[2])) continue;
        out[i] = r[0] >= r[1] && r[0] >= r[2] ? 0 : r[1] >= r[2] ? 1 : 2;
    }
    return out;
}

struct DonorGenotypes {
    std::vector<std::string> names;  // [D] the sample columns of the donor VCF's #CHROM line
    std::vector<uint8_t> gt;         // [D][total_loci], made (all 3) at that line, filled by the records behind it
    uint64_t total_loci = 0;
    std::string field;               // "" (GT alone), or "GP", "GL", "PL": set before the donor lines; then gp is filled too
    std::vector<float> gp;           // [D][total_loci][3], made (all NaN) at the #CHROM line: a sample's weights, else the one-hot of
                                     // its GT, else three NaN; a record with ref and alt swapped has its three values reversed

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
                if (!field.empty()) gp.assign(names.size() * total_loci * 3, std::numeric_limits<float>::quiet_NaN());
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
        int fi = -1;
        for (size_t i = 0; i < fmt.size() && !field.empty(); i++)
            if (fmt[i] == field) { fi = (int)i; break; }
        const char kind = field == "GL" ? 'L' : field == "PL" ? 'Q' : 'P';
        for (size_t d = 0; d < names.size(); d++) {
            const uint8_t g = 9 + d < t.size() ? donor_parse_gt(t[9 + d], gi) : DONOR_NO_CALL;
            gt[d * total_loci + at->second] = g == DONOR_NO_CALL || !swap ? g : (uint8_t)(2 - g);
            if (field.empty()) continue;
            const double nan = std::numeric_limits<double>::quiet_NaN();
            double v[3] = {nan, nan, nan};
            if (!(9 + d < t.size() && donor_parse_weights(t[9 + d], fi, kind, v)) && g != DONOR_NO_CALL)
                for (int k = 0; k < 3; k++) v[k] = k == (int)g ? 1.0 : 0.0;
            float *row = gp.data() + (d * total_loci + at->second) * 3;
            for (int k = 0; k < 3; k++) row[k] = (float)v[swap ? 2 - k : k];
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
