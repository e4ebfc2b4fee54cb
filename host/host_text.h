// Text plumbing shared by the two host binaries (cellector.cpp, combiner.cpp): the exit path of a refusal, Rust's `{}`
// formatting, the line readers over (possibly gzipped) files and the writers of the output files.
#pragma once
#include <zlib.h>

#include <algorithm>
#include <charconv>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <string_view>
#include <thread>
#include <vector>

constexpr int EXIT_PANIC = 101;  // what a Rust panic gives the caller (cellector_pipeline.py checks != 0 only)
[[noreturn]] inline void die(int code, const std::string &msg)
{
    fprintf(stderr, "%s\n", msg.c_str());
    exit(code);
}

// ---- Rust `{}` formatting of f64: shortest round-trip digits, never scientific --------
inline std::string fmt(double v)
{
    if (std::isnan(v)) return "NaN";
    if (std::isinf(v)) return v > 0 ? "inf" : "-inf";
    char buf[400];
    auto r = std::to_chars(buf, buf + sizeof buf, v, std::chars_format::fixed);
    return std::string(buf, r.ptr);
}
inline std::string fmt(uint64_t v) { return std::to_string(v); }
// the same, appended to a row under construction
inline void put(std::string &o, double v)
{
    if (std::isnan(v)) { o += "NaN"; return; }
    if (std::isinf(v)) { o += v > 0 ? "inf" : "-inf"; return; }
    char buf[400];
    auto r = std::to_chars(buf, buf + sizeof buf, v, std::chars_format::fixed);
    o.append(buf, r.ptr);
}
inline void put(std::string &o, uint64_t v)
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

// ---- reader (load_data.rs:240-251, combiner main.rs:233-244): ".gz" by extension, multi-member ----------------
struct Lines {
    gzFile gz = nullptr;
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
inline std::string read_whole(const std::string &path)
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
inline std::vector<std::string_view> split_lines(const std::string &text)
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

inline std::vector<std::string> split(const std::string &s, char sep)
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

// statrs Data::median on a copy (main.rs:442-443); NaN for empty data
inline double median_of(std::vector<double> v)
{
    if (v.empty()) return NAN;
    std::sort(v.begin(), v.end());
    const size_t k = v.size() / 2;
    return v.size() % 2 ? v[k] : (v[k - 1] + v[k]) / 2.0;
}

// an output file, with a 1 MB stdio buffer of its own for the first 64 of a process
inline FILE *create(const std::string &path)
{
    FILE *f = fopen(path.c_str(), "w");
    if (!f) die(EXIT_PANIC, "Unable to create file " + path);
    static std::vector<char> *bufs = new std::vector<char>[64];
    static int nb = 0;
    if (nb < 64) { bufs[nb].resize(1 << 20); setvbuf(f, bufs[nb].data(), _IOFBF, bufs[nb].size()); nb++; }
    return f;
}
// a whole TSV: the header as given (its "\n" included), then rows [0, n) through write_rows
template <class F>
void write_tsv(const std::string &path, const std::string &header, uint64_t n, F row)
{
    FILE *f = create(path);
    fputs(header.c_str(), f);
    write_rows(f, n, row);
    fclose(f);
}
