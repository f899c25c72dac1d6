// purity_emu.cpp — sage_amd/csrc/purity.h compiled for the host: every query of a world through purity::evaluate, one peak after
// another.  Built two ways by tests/test_purity_cpu.py: as a shared library (emu_purity, held bit for bit to
// tests/purity_reference.py, and timed by scripts/purity_bench.py), and with -DPURITY_EMU_MAIN as a program of its own under
// AddressSanitizer and UndefinedBehaviorSanitizer, which reads worlds from files:
//     u64 n_spectra, u64 n_queries, f32 ppm, f32 default_lo, f32 default_hi, u32 max_isotope, u32 has_offsets, u32 0,
//     u64 peak_off[n_spectra + 1], f32 mz[], f32 intensity[], u64 ms1_index[n_queries], f32 precursor_mz[], u8 charge[],
//     then with has_offsets: f32 isolation_lo[], f32 isolation_hi[]
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../sage_amd/csrc/purity.h"

// Returns 0; 1: an ms1_index out of range.  isolation_lo / isolation_hi: either null = the default pair for every query.
extern "C" int emu_purity(uint64_t n_spectra, const uint64_t* peak_off, const float* mz, const float* intensity, uint64_t n_queries,
                          const uint64_t* ms1_index, const float* precursor_mz, const uint8_t* charge, const float* isolation_lo,
                          const float* isolation_hi, float ppm, float default_lo, float default_hi, uint32_t max_isotope,
                          uint32_t* n_window, uint32_t* n_matched, double* total, double* matched, double* below, float* out_purity) {
    const purity::Settings st{ppm, default_lo, default_hi, max_isotope};
    const bool given = isolation_lo && isolation_hi;
    for (uint64_t i = 0; i < n_queries; ++i) {
        const uint64_t s = ms1_index[i];
        purity::Result r = purity::no_result();
        if (s != purity::NO_MS1) {
            if (s >= n_spectra) return 1;
            const uint64_t a = peak_off[s];
            r = purity::evaluate(mz + a, intensity + a, peak_off[s + 1] - a, precursor_mz[i], charge[i],
                                 given ? isolation_lo[i] : __builtin_nanf(""), given ? isolation_hi[i] : __builtin_nanf(""), st);
        }
        n_window[i] = r.n_window;
        n_matched[i] = r.n_matched;
        total[i] = r.total;
        matched[i] = r.matched;
        below[i] = r.below;
        out_purity[i] = r.purity;
    }
    return 0;
}

#ifdef PURITY_EMU_MAIN
template <class T>
static bool read(FILE* fh, std::vector<T>& v, size_t n) {
    v.resize(n);
    return !n || std::fread(v.data(), sizeof(T), n, fh) == n;
}

int main(int argc, char** argv) {
    int worlds = 0;
    for (int i = 1; i < argc; ++i) {
        FILE* fh = std::fopen(argv[i], "rb");
        if (!fh) {
            std::printf("FAILED: cannot open %s\n", argv[i]);
            return 1;
        }
        uint64_t n[2] = {0, 0};
        float f[3] = {0, 0, 0};
        uint32_t u[3] = {0, 0, 0};
        std::vector<uint64_t> off, idx;
        std::vector<float> mz, it, pmz, lo, hi;
        std::vector<uint8_t> z;
        bool ok = std::fread(n, 8, 2, fh) == 2 && std::fread(f, 4, 3, fh) == 3 && std::fread(u, 4, 3, fh) == 3 && read(fh, off, n[0] + 1);
        ok = ok && read(fh, mz, off[n[0]]) && read(fh, it, off[n[0]]) && read(fh, idx, n[1]) && read(fh, pmz, n[1]) && read(fh, z, n[1]);
        if (ok && u[1]) ok = read(fh, lo, n[1]) && read(fh, hi, n[1]);
        std::fclose(fh);
        if (!ok) {
            std::printf("FAILED: %s is cut short\n", argv[i]);
            return 1;
        }
        const size_t q = n[1];
        std::vector<uint32_t> nw(q), nm(q), nw2(q), nm2(q);
        std::vector<double> t(q), m(q), b(q), t2(q), m2(q), b2(q);
        std::vector<float> p(q), p2(q);
        const int rc = emu_purity(n[0], off.data(), mz.data(), it.data(), q, idx.data(), pmz.data(), z.data(), u[1] ? lo.data() : nullptr,
                                  u[1] ? hi.data() : nullptr, f[0], f[1], f[2], u[0], nw.data(), nm.data(), t.data(), m.data(), b.data(),
                                  p.data());
        // once more with the queries in reverse: a query's result must not depend on the others
        std::vector<uint64_t> ridx(idx.rbegin(), idx.rend());
        std::vector<float> rpmz(pmz.rbegin(), pmz.rend()), rlo(lo.rbegin(), lo.rend()), rhi(hi.rbegin(), hi.rend());
        std::vector<uint8_t> rz(z.rbegin(), z.rend());
        const int rc2 = emu_purity(n[0], off.data(), mz.data(), it.data(), q, ridx.data(), rpmz.data(), rz.data(), u[1] ? rlo.data() : nullptr,
                                   u[1] ? rhi.data() : nullptr, f[0], f[1], f[2], u[0], nw2.data(), nm2.data(), t2.data(), m2.data(),
                                   b2.data(), p2.data());
        bool same = rc == 0 && rc2 == 0;
        for (size_t k = 0; same && k < q; ++k) {
            const size_t r = q - 1 - k;
            same = nw[k] == nw2[r] && nm[k] == nm2[r] && !std::memcmp(&t[k], &t2[r], 8) && !std::memcmp(&m[k], &m2[r], 8) &&
                   !std::memcmp(&b[k], &b2[r], 8) && !std::memcmp(&p[k], &p2[r], 4);
        }
        if (!same) {
            std::printf("FAILED: %s: status %d / %d, or results that depend on the order of the queries\n", argv[i], rc, rc2);
            return 1;
        }
        ++worlds;
    }
    std::printf("purity_emu ok (%d worlds)\n", worlds);
    return 0;
}
#endif
