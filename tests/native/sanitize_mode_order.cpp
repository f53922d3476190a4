// Driver for the AddressSanitizer/UBSan build of the mode ordering's row function (bisip_amd/csrc/mode_order.h, plain C++
// when no HIP compiler reads it); built and run by tests/test_modes.py.  Every buffer has exactly the size the entry point
// may touch, so that a read or a write beyond it is reported: rows behind an offset and a stride, every mode count, every
// key group, every combination of outputs, hostile keys (ties, signed zeros, infinities, NaN) among the rows.
#include <cmath>
#include <cstdio>
#include <vector>

#include "../../bisip_amd/csrc/mode_order.h"

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

bool before_or_tie(double a, double b) { return !(b < a) && !(a != a && b == b); }      // a may stand before b

template <int K>
int check(int key_group, int outputs)
{
    constexpr int ND = 1 + 3 * K, NDESC = 1 + 2 * K;
    const int64_t n = 3, rows = 7, pad = 5, offset = 11;
    const int64_t stride = rows * ND + pad;
    std::vector<double> chain((size_t)(offset + (n - 1) * stride + rows * ND));         // ends with the last row
    for (double &v : chain) v = uniform(0.0, 1.0);
    double *key0 = &chain[(size_t)(offset + 1 + key_group * K)];                          // the keys of the first rows
    key0[0] = NAN;                                                                      // row 0: one NaN
    for (int j = 0; j < K; ++j) key0[ND + j] = NAN;                                     // row 1: all NaN
    for (int j = 0; j < K; ++j) key0[2 * ND + j] = j % 2 ? 0.0 : -0.0;                  // row 2: signed zeros, all ties
    key0[3 * ND] = INFINITY;                                                            // row 3: +inf first
    key0[4 * ND + K - 1] = -INFINITY;                                                   // row 4: -inf last
    chain[(size_t)(offset + 5 * ND + 1)] = 1.0;                                           // row 5: m_1 = 1
    chain[(size_t)(offset + 5 * ND + 1 + 2 * K)] = 0.0;                                   //        c_1 = 0
    std::vector<double> ordered(outputs & 1 ? (size_t)(n * rows * ND) : 0, -7.25);
    std::vector<double> desc(outputs & 2 ? (size_t)(n * rows * NDESC) : 0, -7.25);
    std::vector<unsigned char> moved(outputs & 4 ? (size_t)(n * rows) : 0, 9);
    bisip::mode_order_rows_host<K>(chain.data() + offset, n, stride, rows, key_group, outputs & 1 ? ordered.data() : nullptr,
                                   outputs & 2 ? desc.data() : nullptr, outputs & 4 ? moved.data() : nullptr);
    int fails = 0;
    for (int64_t s = 0; s < n; ++s)
        for (int64_t r = 0; r < rows; ++r) {
            const double *in = &chain[(size_t)(offset + s * stride + r * ND)];
            const int64_t at = s * rows + r;
            bool sorted_in = true;
            for (int j = 1; j < K; ++j) sorted_in = sorted_in && before_or_tie(in[key_group * K + j], in[1 + key_group * K + j]);
            if (outputs & 1) {
                const double *o = &ordered[(size_t)(at * ND)];
                if (o[0] != in[0]) ++fails;
                for (int j = 1; j < K; ++j)
                    if (!before_or_tie(o[key_group * K + j], o[1 + key_group * K + j])) ++fails;
                double si = 0.0, so = 0.0;                                              // a permutation keeps the finite sums
                for (int k = 1; k < ND; ++k) {
                    if (std::isfinite(in[k])) si += 1.0;
                    if (std::isfinite(o[k])) so += 1.0;
                }
                if (si != so) ++fails;
            }
            if (outputs & 4) {
                if (moved[(size_t)at] > 1) ++fails;
                if (sorted_in && moved[(size_t)at] != 0) ++fails;                       // already in order: ties keep their places
                if (!sorted_in && moved[(size_t)at] != 1) ++fails;
            }
            if ((outputs & 2) && s == 0 && r == 2 && key_group == 0 && desc[(size_t)(at * NDESC)] != 0.0) ++fails;   // m_total of zeros
        }
    return fails;
}

template <int K>
int check_all()
{
    int fails = 0;
    for (int key_group = 0; key_group < 3; ++key_group)
        for (int outputs = 1; outputs < 8; ++outputs) fails += check<K>(key_group, outputs);
    return fails;
}

}  // namespace

int main()
{
    const int fails = check_all<1>() + check_all<2>() + check_all<3>() + check_all<4>() + check_all<5>();
    std::printf(fails ? "sanitize_mode_order: %d failures\n" : "sanitize_mode_order: ok\n", fails);
    return fails != 0;
}
