// Driver for the AddressSanitizer/UBSan build of the relaxation descriptors' row function
// (bisip_amd/csrc/rtd_descriptors.h, plain C++ when no HIP compiler reads it); built and run by
// tests/test_relaxation.py.  Every buffer has exactly the size the entry point may touch, so that a read or a write
// beyond it is reported: rows behind an offset and a stride, every ndim, L = 1, 2, 40, 64, one to eight fractions.
#include <cmath>
#include <cstdio>
#include <vector>

#include "../../bisip_amd/csrc/rtd_descriptors.h"

namespace {

unsigned long long state = 0x9E3779B97F4A7C15ull;

double uniform(double lo, double hi)        // xorshift64*: the rows need to differ, not to be random
{
    state ^= state >> 12;
    state ^= state << 25;
    state ^= state >> 27;
    const double u = (double)((state * 0x2545F4914F6CDD1Dull) >> 11) / 9007199254740992.0;
    return lo + (hi - lo) * u;
}

int check(int ndim, int L, int nq)
{
    const int64_t n = 3, rows = 7, pad = 5, offset = 11;
    const int64_t stride = rows * ndim + pad;
    std::vector<double> chain((size_t)(offset + (n - 1) * stride + rows * ndim));     // ends with the last row
    for (double &v : chain) v = uniform(-1.0, 1.0);
    chain[offset + 1] = NAN;                                                          // a NaN coefficient
    for (int p = 1; p < ndim; ++p) chain[offset + ndim + p] = p == 1 ? -1.0 : 0.0;      // m_l = -1: no positive RTD
    std::vector<double> x((size_t)L), q((size_t)nq), out((size_t)(n * rows * (2 + nq)), -7.25);
    for (int l = 0; l < L; ++l) x[(size_t)l] = L == 1 ? -6.0 : -6.0 + 8.0 * l / (L - 1);
    for (int j = 0; j < nq; ++j) q[(size_t)j] = (j + 1.0) / nq;                         // the last is 1
    if (!bisip::rtd_descriptor_rows_host_by_ndim<16>(ndim, chain.data() + offset, n, stride, rows, x.data(), L, q.data(), nq,
                                                     out.data()))
        return 1;
    int fails = 0;
    for (int64_t r = 0; r < n * rows; ++r) {
        const double *o = &out[(size_t)(r * (2 + nq))];
        const bool nan = o[0] != o[0];
        for (int k = 0; k < 2 + nq; ++k) {
            if ((o[k] != o[k]) != nan) ++fails;                                       // a row is NaN throughout or nowhere
            if (!nan && k != 1 && !(o[k] >= x[0] && std::isfinite(o[k]))) ++fails;      // fma(f >= 0, step, x_{k-1}) >= x_0
        }
    }
    if (!(out[0] != out[0])) ++fails;                                                 // the row with the NaN coefficient
    if (!(out[(size_t)(2 + nq)] != out[(size_t)(2 + nq)])) ++fails;                   // the row with no positive RTD
    return fails;
}

}  // namespace

int main()
{
    int fails = 0;
    const int Ls[] = {1, 2, 40, 64};
    for (int ndim = 2; ndim <= 16; ++ndim)
        for (int L : Ls)
            for (int nq = 1; nq <= bisip::RTD_MAX_FRACTIONS; ++nq) fails += check(ndim, L, nq);
    double none[1] = {0.0};
    if (bisip::rtd_descriptor_rows_host_by_ndim<16>(17, none, 1, 17, 1, none, 1, none, 1, none)) ++fails;   // refused, nothing read
    if (bisip::rtd_descriptor_rows_host_by_ndim<16>(1, none, 1, 1, 1, none, 1, none, 1, none)) ++fails;
    std::printf(fails ? "sanitize_rtd_descriptors: %d failures\n" : "sanitize_rtd_descriptors: ok\n", fails);
    return fails != 0;
}
