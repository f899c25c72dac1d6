// mgf_reader.cpp — MGF input on the host, in C++ (.mgf and .mgf.gz).
//
// Follows crates/sage-cloudpath/src/mgf.rs (MgfReader::parse, :325-369) line for line, quirks included:
//   * lines are `str::lines()` pieces (split at '\n', one trailing '\r' dropped), each `trim()`med (Unicode White_Space);
//   * the file-level section is everything before the first line that starts with `BEGIN IONS` (:333-352): `TOL=`, `TOLU=` and
//     `CHARGE=` there set defaults.  A file without `BEGIN IONS` is an error here (the reference panics at `lines.next().unwrap()`);
//   * the defaults do NOT apply to the first spectrum: QueryData::default_with_params (:55-60) does not call init(); only the
//     init() at `END IONS` (:61-70, :316) copies them in;
//   * `BEGIN IONS` matches no query parser (:185-196): state is reset only at `END IONS`, so lines between one `END IONS` and
//     the next `BEGIN IONS` belong to the next spectrum;
//   * the query parsers run in the order mz, end, pepmass, title, charge, tol, tolu, rt; the first Ok(true) wins;
//   * a peak line starts with a digit (:276-299): m/z that does not parse adds nothing; a missing intensity is 1.0; an intensity
//     that does not parse leaves the arrays of different lengths (the spectrum is then dropped at `END IONS`);
//   * `PEPMASS=` (:198-221): the first token is the m/z (none: 0, unparsable: no precursor), the second the intensity;
//   * `CHARGE=` (:223-236): one charge per match of `(\d)\+?` whose digit is ASCII (`to_digit(10)`), so `10+` is [1, 0];
//     precursors are PEPMASS x charge (:86-104) and only precursors[0] is read by the search;
//   * isolation window (:72-83): `TOL` and `TOLU` both set and the unit exactly `Da` or `ppm`; else None;
//   * `RTINSECONDS=` in minutes (f32 / 60), `TITLE=` verbatim; check_spectrum (:115-128) drops a spectrum with an empty id, no
//     precursor, no peaks or peak arrays of different lengths, with a message, and the rest of the file is read;
//   * every number goes through `str::parse::<f32>()`: parse_f32_rust below.
// The query section is parsed in parallel pieces cut after `END IONS` lines.  State crosses a spectrum boundary only through the
// file defaults (init()), so a piece that starts behind an `END IONS` starts in exactly the state the sequential parse has there;
// the first piece starts in the no-defaults state.  Spectra come out in file order.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <string_view>
#include <vector>

#include "host_db.hpp"

namespace sagehip {

// Rust's f32::from_str: [+-]? ( 'inf' | 'infinity' | 'nan' | Digit+ | Digit+ '.' Digit* | Digit* '.' Digit+ ) ( [eE] [+-]? Digit+ )?
// (the keywords and the exponent letter in any case), nothing else — no surrounding whitespace, no hex, no `nan(...)`.  The value
// is correctly rounded, as glibc's strtof is for every string of this grammar.
bool parse_f32_rust(const char* b, const char* e, float& out) {
    const char* p = b;
    if (p < e && (*p == '+' || *p == '-')) p++;
    const size_t rest = (size_t)(e - p);
    auto ieq = [&](const char* word) {
        const size_t n = std::strlen(word);
        if (rest != n) return false;
        for (size_t i = 0; i < n; i++)
            if ((char)(p[i] | 0x20) != word[i]) return false;
        return true;
    };
    if (!(ieq("inf") || ieq("infinity") || ieq("nan"))) {
        size_t digits = 0;
        while (p < e && *p >= '0' && *p <= '9') p++, digits++;
        if (p < e && *p == '.') {
            p++;
            while (p < e && *p >= '0' && *p <= '9') p++, digits++;
        }
        if (!digits) return false;
        if (p < e && (*p == 'e' || *p == 'E')) {
            p++;
            if (p < e && (*p == '+' || *p == '-')) p++;
            size_t exp_digits = 0;
            while (p < e && *p >= '0' && *p <= '9') p++, exp_digits++;
            if (!exp_digits) return false;
        }
        if (p != e) return false;
    }
    char small[64];
    const size_t n = (size_t)(e - b);
    if (n < sizeof(small)) {
        std::memcpy(small, b, n);
        small[n] = '\0';
        out = std::strtof(small, nullptr);
    } else {
        out = std::strtof(std::string(b, n).c_str(), nullptr);
    }
    return true;
}

namespace {

// char::is_whitespace (Unicode White_Space) at the front / back of [b, e): the byte length of that character, 0 if none
size_t ws_front(const char* b, const char* e) {
    const unsigned char c = (unsigned char)*b;
    if (c == ' ' || (c >= 0x09 && c <= 0x0D)) return 1;
    const size_t n = (size_t)(e - b);
    const unsigned char* u = (const unsigned char*)b;
    if (n >= 2 && u[0] == 0xC2 && (u[1] == 0x85 || u[1] == 0xA0)) return 2;
    if (n >= 3) {
        if (u[0] == 0xE1 && u[1] == 0x9A && u[2] == 0x80) return 3;                                   // U+1680
        if (u[0] == 0xE2 && u[1] == 0x80 && (u[2] <= 0x8A || u[2] == 0xA8 || u[2] == 0xA9 || u[2] == 0xAF)) return 3;  // U+2000-200A, 2028, 2029, 202F
        if (u[0] == 0xE2 && u[1] == 0x81 && u[2] == 0x9F) return 3;                                   // U+205F
        if (u[0] == 0xE3 && u[1] == 0x80 && u[2] == 0x80) return 3;                                   // U+3000
    }
    return 0;
}
size_t ws_back(const char* b, const char* e) {
    const unsigned char c = (unsigned char)e[-1];
    if (c == ' ' || (c >= 0x09 && c <= 0x0D)) return 1;
    const size_t n = (size_t)(e - b);
    if (n >= 2 && ws_front(e - 2, e) == 2) return 2;
    if (n >= 3 && ws_front(e - 3, e) == 3) return 3;
    return 0;
}
std::string_view trim(const char* b, const char* e) {
    while (b < e) {
        const size_t k = ws_front(b, e);
        if (!k) break;
        b += k;
    }
    while (b < e) {
        const size_t k = ws_back(b, e);
        if (!k) break;
        e -= k;
    }
    return std::string_view(b, (size_t)(e - b));
}
bool starts(std::string_view s, std::string_view prefix) { return s.size() >= prefix.size() && s.substr(0, prefix.size()) == prefix; }

// u8::is_ascii_whitespace (split_ascii_whitespace): space, \t, \n, \x0C, \r — not \x0B
bool ascii_ws(char c) { return c == ' ' || c == '\t' || c == '\n' || c == '\x0C' || c == '\r'; }
// the next split_ascii_whitespace token of s from `at`; false when none is left
bool next_token(std::string_view s, size_t& at, std::string_view& tok) {
    while (at < s.size() && ascii_ws(s[at])) at++;
    if (at >= s.size()) return false;
    const size_t b = at;
    while (at < s.size() && !ascii_ws(s[at])) at++;
    tok = s.substr(b, at - b);
    return true;
}
bool f32_of(std::string_view s, float& out) { return parse_f32_rust(s.data(), s.data() + s.size(), out); }

// String::from_utf8 / read_to_string: the text must be valid UTF-8
bool valid_utf8(const char* b, const char* e) {
    const unsigned char* p = (const unsigned char*)b;
    const unsigned char* q = (const unsigned char*)e;
    while (p < q) {
        if (*p < 0x80) {
            p++;
            continue;
        }
        size_t n;
        uint32_t cp;
        if ((*p & 0xE0) == 0xC0) n = 2, cp = *p & 0x1F;
        else if ((*p & 0xF0) == 0xE0) n = 3, cp = *p & 0x0F;
        else if ((*p & 0xF8) == 0xF0) n = 4, cp = *p & 0x07;
        else return false;
        if ((size_t)(q - p) < n) return false;
        for (size_t i = 1; i < n; i++) {
            if ((p[i] & 0xC0) != 0x80) return false;
            cp = (cp << 6) | (p[i] & 0x3F);
        }
        if ((n == 2 && cp < 0x80) || (n == 3 && cp < 0x800) || (n == 4 && cp < 0x10000) || cp > 0x10FFFF ||
            (cp >= 0xD800 && cp <= 0xDFFF))
            return false;
        p += n;
    }
    return true;
}

// `CHARGE=` (mgf.rs:223-236): regex (\d)\+? over the value; each match's digit, if ASCII (to_digit(10)), is a charge
std::vector<uint8_t> charges_of(std::string_view s) {
    std::vector<uint8_t> c;
    for (char ch : s)
        if (ch >= '0' && ch <= '9') c.push_back((uint8_t)(ch - '0'));
    return c;
}

struct Defaults {
    bool has_tol = false;
    float tol = 0.0f;
    bool has_unit = false;
    std::string unit;
    bool has_charges = false;
    std::vector<uint8_t> charges;
};

struct Spectrum {
    std::string id;
    float prec_mz = 0.0f, iso_lo = NAN, iso_hi = NAN, rt = 0.0f;
    uint8_t charge = 0, charge_zero = 0, iso_kind = SAGE_TOL_DA;
    std::vector<float> mz, inten;
};

// QueryData (mgf.rs:39-129) over one piece of the query section
struct Query {
    const Defaults& d;
    std::string id;
    std::vector<float> prec_mz;  // precursors (their intensities are read by nothing downstream)
    bool has_tol = false;
    float tol = 0.0f;
    bool has_unit = false;
    std::string unit;
    bool has_charges = false;
    std::vector<uint8_t> charges;
    bool has_rt = false;
    float rt = 0.0f;
    std::vector<float> mz, inten;
    std::vector<Spectrum> out;
    std::vector<std::string> dropped;  // ids of the spectra check_spectrum refused, in order

    explicit Query(const Defaults& defaults) : d(defaults) {}
    void init() {  // :61-70
        id.clear();
        prec_mz.clear();
        has_tol = d.has_tol, tol = d.tol;
        has_unit = d.has_unit, unit = d.unit;
        has_charges = d.has_charges, charges = d.charges;
        has_rt = false, rt = 0.0f;
        mz.clear();
        inten.clear();
    }
    void end() {  // parse_end, :301-320
        const bool has_precursor = !prec_mz.empty() && !(has_charges && charges.empty());
        if (id.empty() || !has_precursor || mz.empty() || mz.size() != inten.size()) {
            dropped.push_back(id);
        } else {
            Spectrum s;
            s.id = id;
            s.prec_mz = prec_mz[0];
            if (has_charges) {
                s.charge = charges[0];
                s.charge_zero = charges[0] == 0;
            }
            if (has_tol && has_unit && (unit == "Da" || unit == "ppm")) {  // get_isolation_window, :72-83
                s.iso_kind = unit == "Da" ? SAGE_TOL_DA : SAGE_TOL_PPM;
                s.iso_lo = -std::fabs(tol);
                s.iso_hi = std::fabs(tol);
                if (tol != tol) {  // Da(NaN, NaN): bounds that match nothing; NaN bounds would read as None (+-2.4 Da)
                    s.iso_lo = INFINITY;
                    s.iso_hi = -INFINITY;
                }
            }
            s.rt = has_rt ? rt : 0.0f;
            s.mz.swap(mz);
            s.inten.swap(inten);
            out.push_back(std::move(s));
        }
        init();
    }
    void line(std::string_view l) {
        if (!l.empty() && l[0] >= '0' && l[0] <= '9') {  // parse_mz (a line led by a non-ASCII numeric char fails to parse: nothing)
            size_t at = 0;
            std::string_view tok;
            float v;
            next_token(l, at, tok);
            if (!f32_of(tok, v)) return;
            mz.push_back(v);
            if (next_token(l, at, tok)) {
                if (f32_of(tok, v)) inten.push_back(v);
            } else {
                inten.push_back(1.0f);
            }
            return;
        }
        if (starts(l, "END IONS")) return end();
        if (starts(l, "PEPMASS=")) {
            std::string_view rest = l.substr(8), tok;
            size_t at = 0;
            float v = 0.0f;
            if (next_token(rest, at, tok) && !f32_of(tok, v)) return;  // Err: no precursor
            prec_mz.push_back(v);
            return;
        }
        if (starts(l, "TITLE=")) {
            id.assign(l.substr(6));
            return;
        }
        if (starts(l, "CHARGE=")) {
            has_charges = true;
            charges = charges_of(l.substr(7));
            return;
        }
        if (starts(l, "TOL=")) {
            float v;
            if (f32_of(l.substr(4), v)) has_tol = true, tol = v;
            return;
        }
        if (starts(l, "TOLU=")) {
            has_unit = true;
            unit.assign(l.substr(5));
            return;
        }
        if (starts(l, "RTINSECONDS=")) {
            float v;
            if (f32_of(l.substr(12), v)) has_rt = true, rt = v / 60.0f;
            return;
        }
    }
};

// str::lines(): [b, e) cut at '\n', one trailing '\r' dropped; calls f(line_begin, line_end, next_line_begin)
template <typename F>
void each_line(const char* b, const char* e, F&& f) {
    while (b < e) {
        const char* nl = (const char*)std::memchr(b, '\n', (size_t)(e - b));
        const char* le = nl ? nl : e;
        const char* next = nl ? nl + 1 : e;
        const char* te = (le > b && le[-1] == '\r') ? le - 1 : le;
        if (!f(b, te, next)) return;
        b = next;
    }
}

}  // namespace

bool read_mgf(const char* path, uint32_t file_id, MzmlRun& run, std::string& err) {
    std::string text;
    if (!load_text(path, text, err)) return false;
    const char *p = text.data(), *e = text.data() + text.size();
    // file-level section (:333-352)
    Defaults d;
    const char* query = nullptr;
    each_line(p, e, [&](const char* b, const char* le, const char* next) {
        const std::string_view l = trim(b, le);
        if (starts(l, "BEGIN IONS")) {
            query = next;
            return false;
        }
        float v;
        if (starts(l, "TOL=")) {
            if (f32_of(l.substr(4), v)) d.has_tol = true, d.tol = v;
        } else if (starts(l, "TOLU=")) {
            d.has_unit = true;
            d.unit.assign(l.substr(5));
        } else if (starts(l, "CHARGE=")) {
            d.has_charges = true;
            d.charges = charges_of(l.substr(7));
        }
        return true;
    });
    if (!valid_utf8(p, query ? query : e)) {
        err = std::string("stream did not contain valid UTF-8: ") + path;
        return false;
    }
    if (!query) {
        err = std::string("malformed MGF: no BEGIN IONS in ") + path;
        return false;
    }
    // pieces of the query section, each cut behind an `END IONS` line at or after a multiple of the piece size
    size_t piece = (size_t)4 << 20;
    if (const char* v = std::getenv("SAGE_HIP_MGF_PIECE_KB")) piece = (size_t)std::max(1, std::atoi(v)) << 10;  // (tests)
    std::vector<const char*> cuts{query};
    if ((size_t)(e - query) >= 2 * piece && host_threads() > 1) {
        const char* at = query + piece;
        while (at < e) {
            const char* nl = (const char*)std::memchr(at, '\n', (size_t)(e - at));  // (the line `at` falls in is not a cut)
            if (!nl) break;
            const char* cut = nullptr;
            each_line(nl + 1, e, [&](const char* b, const char* le, const char* next) {
                if (starts(trim(b, le), "END IONS")) {
                    cut = next;
                    return false;
                }
                return true;
            });
            if (!cut || cut >= e) break;
            cuts.push_back(cut);
            at = std::max(cut, at + piece);
        }
    }
    const size_t n_pieces = cuts.size();
    std::vector<Query> parts;
    parts.reserve(n_pieces);
    for (size_t k = 0; k < n_pieces; k++) parts.emplace_back(d);
    std::vector<uint8_t> bad_utf8(n_pieces, 0);
    parallel_for(n_pieces, 1, [&](size_t b, size_t e2, unsigned) {
        for (size_t k = b; k < e2; k++) {
            const char* from = cuts[k];
            const char* to = k + 1 < n_pieces ? cuts[k + 1] : e;
            if (!valid_utf8(from, to)) {
                bad_utf8[k] = 1;
                continue;
            }
            Query& q = parts[k];
            if (k > 0) q.init();  // behind an `END IONS`: the defaults are in; the first spectrum has none
            each_line(from, to, [&](const char* lb, const char* le, const char* next) {
                if (lb != le) q.line(trim(lb, le));  // (:356-358: empty lines are skipped before trim)
                return true;
            });
        }
    });
    for (uint8_t bad : bad_utf8)
        if (bad) {
            err = std::string("stream did not contain valid UTF-8: ") + path;
            return false;
        }
    size_t n = 0, n_peaks = 0, id_bytes = 0;
    for (const Query& q : parts) {
        for (const std::string& id : q.dropped) std::fprintf(stderr, "malformed MGF: spectrum '%s' in %s dropped\n", id.c_str(), path);
        n += q.out.size();
        for (const Spectrum& s : q.out) n_peaks += s.mz.size(), id_bytes += s.id.size() + 1;
    }
    run = MzmlRun{};
    run.peak_off.reserve(n + 1);
    run.peak_off.push_back(0);
    run.id_off.reserve(n + 1);
    run.id_off.push_back(0);
    run.ids.reserve(id_bytes);
    run.mz.resize(n_peaks);
    run.intensities.resize(n_peaks);
    run.precursor_mz.resize(n);
    run.precursor_charge.resize(n);
    run.isolation_lo.resize(n);
    run.isolation_hi.resize(n);
    run.scan_start_time.resize(n);
    run.ion_injection_time.assign(n, 0.0f);
    run.inverse_ion_mobility.assign(n, NAN);
    run.file_id.assign(n, file_id);
    run.centroid.assign(n, 1);
    run.has_precursor.assign(n, 1);
    run.ms_level.assign(n, 2);
    run.iso_kind.resize(n);
    run.charge_zero.resize(n);
    run.precursor_refs.assign(n, '\0');
    run.ref_off.reserve(n + 1);
    size_t j = 0;
    for (const Query& q : parts)
        for (const Spectrum& s : q.out) {
            const size_t at = run.peak_off.back();
            if (!s.mz.empty()) {
                std::memcpy(run.mz.data() + at, s.mz.data(), s.mz.size() * sizeof(float));
                std::memcpy(run.intensities.data() + at, s.inten.data(), s.inten.size() * sizeof(float));
            }
            run.peak_off.push_back(at + s.mz.size());
            run.precursor_mz[j] = s.prec_mz;
            run.precursor_charge[j] = s.charge;
            run.charge_zero[j] = s.charge_zero;
            run.isolation_lo[j] = s.iso_lo;
            run.isolation_hi[j] = s.iso_hi;
            run.iso_kind[j] = s.iso_kind;
            run.scan_start_time[j] = s.rt;
            run.ids += s.id;
            run.ids += '\0';
            run.id_off.push_back(run.ids.size());
            run.ref_off.push_back(j + 1);
            j++;
        }
    return true;
}

}  // namespace sagehip
