// localise_math.h — the f64 arithmetic of site localisation over the integer counts the device returns (used by
// capi_psm.hip).  Plain C++: no HIP header, so tests/hostemu/localise_math_emu.cpp compiles it by itself.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

// The depth scores of site localisation: S(n, N, d) = -10 log10 P(X >= n), X ~ Binomial(N, d / 100), by log-sum-exp
// over k = n .. N in ascending k (N reaches several hundred, where the plain product underflows).  A search asks for the same
// (n, N, d) again and again — some hundred thousand candidates, a few hundred distinct N —, so every value is computed once, by
// exactly this arithmetic, and kept; lg[k] = ln Gamma(k + 1) = ln k!.
// ln Gamma(x) for x >= 1 by the Lanczos approximation with g = 6.0246800407767296 and 13 terms (the rational form and the
// coefficients of Boost.Math's lanczos13m53, which CPython's math.lgamma evaluates in the same way): the C library's lgamma is
// not used, since it writes the process-wide `signgam` — two scorers localise on two host threads — and its last bits change from
// one C library to the next, and with them the last digits of every score in localisation.sage.tsv.
inline double lgamma_lanczos(double x) {
    static const double NUM[13] = {23531376880.410759688572007674451636754734846804940, 42919803642.649098768957899047001988850926355848959,
                                   35711959237.355668049440185451547166705960488635843, 17921034426.037209699919755754458931112671403265390,
                                   6039542586.3520280050642916443072979210699388420708, 1439720407.3117216736632230727949123939715485786772,
                                   248874557.86205415651146038641322942321632125127801, 31426415.585400194380614231628318205362874684987640,
                                   2876370.6289353724412254090516208496135991145378768, 186056.26539522349504029498971604569928220784236328,
                                   8071.6720023658162106380029022722506138218516325024, 210.82427775157934587250973392071336271166969580291,
                                   2.5066282746310002701649081771338373386264310793408};
    static const double DEN[13] = {0.0, 39916800.0, 120543840.0, 150917976.0, 105258076.0, 45995730.0, 13339535.0, 2637558.0,
                                   357423.0, 32670.0, 1925.0, 66.0, 1.0};
    const double g = 6.024680040776729583740234375;
    if (x == 1.0 || x == 2.0) return 0.0;
    double num = 0.0, den = 0.0;
    if (x < 5.0) {
        for (int i = 12; i >= 0; i--) {
            num = num * x + NUM[i];
            den = den * x + DEN[i];
        }
    } else {  // (in 1 / x: the powers of a large x would overflow)
        for (int i = 0; i < 13; i++) {
            num = num / x + NUM[i];
            den = den / x + DEN[i];
        }
    }
    double r = std::log(num / den) - g;
    r += (x - 0.5) * (std::log(x + g - 0.5) - 1.0);
    return r;
}
constexpr uint32_t LOC_NONE = 0xFFFFFFFFu;
const double LOC_WEIGHT[10] = {0.5, 0.75, 1.0, 1.0, 1.0, 1.0, 0.75, 0.5, 0.25, 0.25};
struct DepthScores {
    std::vector<double> lg, terms;
    std::vector<std::vector<double>> by_n_items;  // [N][(n - 1) * 10 + d - 1], NaN = not computed yet
    size_t kept = 0;
    double compute(uint32_t n, uint32_t N, uint32_t d) {
        while (lg.size() <= N) lg.push_back(lgamma_lanczos((double)lg.size() + 1.0));
        const double p = (double)d / 100.0, lp = std::log(p), lq = std::log(1.0 - p);
        terms.resize((size_t)N - n + 1);
        double m = -INFINITY;
        for (uint32_t k = n; k <= N; k++) {
            const double v = lg[N] - lg[k] - lg[N - k] + (double)k * lp + (double)(N - k) * lq;
            terms[k - n] = v;
            if (v > m) m = v;
        }
        double sum = 0.0;
        for (double v : terms) sum += std::exp(v - m);
        return -10.0 / std::log(10.0) * (m + std::log(sum));
    }
    double get(uint32_t n, uint32_t N, uint32_t d) {
        if (n == 0 || N == 0) return 0.0;
        if (kept > (1u << 23)) {  // (64 MB of values: start again)
            by_n_items.clear();
            kept = 0;
        }
        if (by_n_items.size() <= N) by_n_items.resize((size_t)N + 1);
        std::vector<double>& t = by_n_items[N];
        if (t.empty()) {
            t.assign((size_t)N * 10, std::nan(""));
            kept += t.size();
        }
        double& v = t[(size_t)(n - 1) * 10 + d - 1];
        if (std::isnan(v)) v = compute(n, N, d);
        return v;
    }
};

inline double peptide_score(DepthScores& ds, const uint16_t* n, uint32_t N) {
    double sum = 0.0;
    for (uint32_t d = 1; d <= 10; d++) sum += LOC_WEIGHT[d - 1] * ds.get(n[d - 1], N, d);
    return sum / 7.0;
}
// d*: the depth with the largest a[d] - b[d] (signed), ties to the smallest; the Ascore there
inline double ascore_of(DepthScores& ds, const uint16_t* a, const uint16_t* b, uint32_t Ns, uint8_t& depth) {
    depth = 1;
    if (Ns == 0) return 0.0;
    int best = (int)a[0] - (int)b[0];
    for (uint32_t d = 2; d <= 10; d++)
        if ((int)a[d - 1] - (int)b[d - 1] > best) {
            best = (int)a[d - 1] - (int)b[d - 1];
            depth = (uint8_t)d;
        }
    return ds.get(a[depth - 1], Ns, depth) - ds.get(b[depth - 1], Ns, depth);
}
