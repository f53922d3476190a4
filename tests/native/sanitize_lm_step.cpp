// Driver for the AddressSanitizer/UBSan build of the Levenberg-Marquardt dense step (bisip_amd/csrc/lm_step.h, plain C++
// when no HIP compiler reads it); built and run by tests/test_mapfit.py.  Every buffer has exactly the size the functions may
// touch, so that a read or a write beyond it is reported: ndim 1, 2 and 16, a positive definite A, a singular A, a free set
// that is empty (every parameter on a bound with the gradient pushing outwards), a parameter of zero sensitivity, NaN in A.
#include <cmath>
#include <cstdio>
#include <vector>

#include "../../bisip_amd/csrc/lm_step.h"

namespace {

unsigned long long state = 0x9E3779B97F4A7C15ull;

double uniform(double lo, double hi)        // xorshift64*: the entries need to differ, not to be random
{
    state ^= state >> 12;
    state ^= state << 25;
    state ^= state >> 27;
    const double u = (double)((state * 0x2545F4914F6CDD1Dull) >> 11) / 9007199254740992.0;
    return lo + (hi - lo) * u;
}

enum Kind { PD, SINGULAR, ALL_FIXED, ZERO_ROW, NAN_ENTRY };

// A = J'J of a random (rows x n) J: positive definite with rows = n + 2; SINGULAR: one row of small non-zero integers, so that
// A = v v' is exact and its second pivot exactly 0 (ndim 1 has no such A: its singular A is the zero of ZERO_ROW)
int check(int n, Kind kind)
{
    const int rows = kind == SINGULAR ? 1 : n + 2;
    std::vector<double> J((size_t)rows * n), A((size_t)n * n, 0.0), g((size_t)n), theta((size_t)n), lo((size_t)n), hi((size_t)n);
    for (double &v : J) v = kind == SINGULAR ? (uniform(0.0, 1.0) < 0.5 ? -1.0 : 1.0) * std::floor(uniform(1.0, 4.0)) : uniform(-1.0, 1.0);
    if (kind == ZERO_ROW)
        for (int r = 0; r < rows; ++r) J[(size_t)r * n + n / 2] = 0.0;
    for (int j = 0; j < n; ++j)
        for (int k = 0; k < n; ++k)
            for (int r = 0; r < rows; ++r) A[(size_t)j * n + k] += J[(size_t)r * n + j] * J[(size_t)r * n + k];
    for (int j = 0; j < n; ++j) {
        lo[j] = -1.0 - j;
        hi[j] = 2.0 + j;
        theta[j] = uniform(lo[j] + 0.1, hi[j] - 0.1);
        g[j] = kind == ZERO_ROW && j == n / 2 ? 0.0 : uniform(-1.0, 1.0);
    }
    if (kind == NAN_ENTRY) A[(size_t)(n - 1) * n] = A[(size_t)n - 1] = NAN;
    std::vector<double> h((size_t)n), lo_in((size_t)n), hi_in((size_t)n);
    bisip::lm_inner_box(n, lo.data(), hi.data(), h.data(), lo_in.data(), hi_in.data());
    if (kind == ALL_FIXED)
        for (int j = 0; j < n; ++j) {
            theta[j] = j % 2 ? hi_in[j] : lo_in[j];
            g[j] = j % 2 ? -1.0 : 1.0;
        }
    int fails = 0;
    for (const double lambda : {0.0, 1e-3, 1e3, 1e9}) {
        std::vector<double> delta((size_t)n, -7.25), trial((size_t)n, -7.25);
        double pred = -7.25;
        int64_t fixed = -1;
        int ok = -1;
        bisip::lm_step_host(n, A.data(), g.data(), theta.data(), lo.data(), hi.data(), lambda, delta.data(), trial.data(), &pred,
                            &fixed, &ok);
        if (ok != 0 && ok != 1) ++fails;
        if (fixed < 0 || fixed >= (int64_t)1 << n) ++fails;
        if (kind == ALL_FIXED) {
            if (fixed != ((int64_t)1 << n) - 1 || pred != 0.0 || ok != 1) ++fails;          // nothing to solve: a step of zero
            for (int j = 0; j < n; ++j)
                if (delta[j] != 0.0 || trial[j] != theta[j]) ++fails;
        }
        if (kind == PD) {
            if (ok != 1 || !(pred > 0.0) || !std::isfinite(pred) || fixed != 0) ++fails;
            // (A + lambda D) delta = -g: the residual is small against |g|
            for (int j = 0; j < n && ok; ++j) {
                double r = g[j];
                for (int k = 0; k < n; ++k) r += (A[(size_t)j * n + k] + (j == k ? lambda * A[(size_t)j * n + j] : 0.0)) * delta[k];
                if (!(std::fabs(r) < 1e-6)) ++fails;
                if (!(trial[j] >= lo_in[j] && trial[j] <= hi_in[j])) ++fails;
            }
        }
        if (kind == SINGULAR && lambda == 0.0 && (ok != 0 || pred != HUGE_VAL)) ++fails;         // not positive definite: pred = +inf
        if (kind == SINGULAR && lambda == 0.0)
            for (int j = 0; j < n; ++j)
                if (!std::isnan(delta[j]) || !std::isnan(trial[j])) ++fails;
        if (kind == SINGULAR && lambda >= 1e3 && n > 1 && ok != 1) ++fails;                      // the damping makes it definite
        if (kind == ZERO_ROW) {
            if (!(fixed >> (n / 2) & 1) || ok != 1 || !std::isfinite(pred)) ++fails;
            if (delta[n / 2] != 0.0) ++fails;
        }
        if (kind == NAN_ENTRY && n > 1 && lambda == 0.0 && (ok != 0 || pred != HUGE_VAL)) ++fails;   // a NaN fails the factorisation
        // null outputs are not written
        bisip::lm_step_host(n, A.data(), g.data(), theta.data(), lo.data(), hi.data(), lambda, nullptr, nullptr, nullptr, nullptr,
                            nullptr);
    }
    return fails;
}

}  // namespace

int main()
{
    int fails = 0;
    for (const int n : {1, 2, 16})
        for (const Kind kind : {PD, SINGULAR, ALL_FIXED, ZERO_ROW, NAN_ENTRY}) {
            if (n == 1 && kind == SINGULAR) continue;                                            // (ZERO_ROW is its singular A)
            const int f = check(n, kind);
            if (f) std::printf("ndim %d kind %d: %d failures\n", n, (int)kind, f);
            fails += f;
        }
    std::printf(fails ? "sanitize_lm_step: %d failures\n" : "sanitize_lm_step: ok\n", fails);
    return fails != 0;
}
