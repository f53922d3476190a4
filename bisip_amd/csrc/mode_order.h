// mode_order.h -- ONE row of a PeltonColeCole chain with its modes put in order, and the per-mode descriptors of the
// ordered row.  The definitions are in the module docstring of bisip_amd/modes.py ("Ordering", "Descriptors"); this is
// their only implementation in C++.  The kernel k_mode_order<K> and the host entry point bisip_mode_order_host
// (chain_modes.hip) both call mode_order_row<K>, so that the device's bits can be held to the host's: the ordered row is
// a pure permutation (copies), m_total a chain of plain additions.  No product is followed by a sum (2 c is followed by
// a division, log1p(-m) / c by the sum with log_tau), so nothing here can be contracted.
// The sort is the optimal compare-exchange network of K = 1 ... 5 values (0, 1, 3, 5, 9 comparators) on (key, original
// index): the index is the second key, which makes the network's result the stable sort's.  Every value has a
// compile-time index -- no array is indexed by a run-time value, so that a kernel keeps all of it in registers.
// Plain C++ when no HIP compiler reads it (tests/native/sanitize_mode_order.cpp builds it with g++).
#pragma once
#include <cmath>
#include <cstdint>

#ifndef BISIP_HD            // as philox.h defines it (a unit may hold both headers): the inline is part of it
#ifdef __HIPCC__
#define BISIP_HD __host__ __device__ __forceinline__
#else
#define BISIP_HD inline
#endif
#endif

namespace bisip {

constexpr int MODE_KEY_M = 0, MODE_KEY_LOG_TAU = 1, MODE_KEY_C = 2;      // key_group of the C ABI

// one mode as the network moves it
struct ModeSlot {
    double key, m, lt, c;
    int src;               // its position in the row as stored
};

// a before b in the order of the key: IEEE <, every NaN after +inf, NaNs (and -0.0, +0.0) tie
BISIP_HD bool mode_key_less(double a, double b) { return a < b || (a == a && b != b); }

// one comparator: afterwards lo is before hi in (key, src).  Value by value, each a select: nothing goes through memory.
BISIP_HD void mode_compare_exchange(ModeSlot &lo, ModeSlot &hi)
{
    const bool swap = mode_key_less(hi.key, lo.key) || (!mode_key_less(lo.key, hi.key) && hi.src < lo.src);
    const double key = lo.key, m = lo.m, lt = lo.lt, c = lo.c;
    const int src = lo.src;
    lo.key = swap ? hi.key : key;
    lo.m = swap ? hi.m : m;
    lo.lt = swap ? hi.lt : lt;
    lo.c = swap ? hi.c : c;
    lo.src = swap ? hi.src : src;
    hi.key = swap ? key : hi.key;
    hi.m = swap ? m : hi.m;
    hi.lt = swap ? lt : hi.lt;
    hi.c = swap ? c : hi.c;
    hi.src = swap ? src : hi.src;
}

template <int K>
BISIP_HD void mode_sort_network(ModeSlot *v)
{
    static_assert(K >= 1 && K <= 5, "networks for 1 ... 5 modes");
#define BISIP_CX(i, j) mode_compare_exchange(v[i], v[j])
    if constexpr (K == 2) {
        BISIP_CX(0, 1);
    } else if constexpr (K == 3) {
        BISIP_CX(0, 2); BISIP_CX(0, 1); BISIP_CX(1, 2);
    } else if constexpr (K == 4) {
        BISIP_CX(0, 2); BISIP_CX(1, 3); BISIP_CX(0, 1); BISIP_CX(2, 3); BISIP_CX(1, 2);
    } else if constexpr (K == 5) {
        BISIP_CX(0, 3); BISIP_CX(1, 4); BISIP_CX(0, 2); BISIP_CX(1, 3); BISIP_CX(0, 1); BISIP_CX(2, 4); BISIP_CX(1, 2);
        BISIP_CX(3, 4); BISIP_CX(2, 3);
    }
#undef BISIP_CX
}

// th: the row (r0, m_1..m_K, log_tau_1..K, c_1..K), 1 + 3K values.  ordered: the row with the modes in ascending order
// of the key group (1 + 3K values, always written: registers in the kernel).  desc: (m_total, log_tau_cc_1..K,
// log_tau_peak_1..K), 1 + 2K values, written only with want_desc.  Returns moved: some mode left its place.
template <int K>
BISIP_HD bool mode_order_row(const double *th, int key_group, double *ordered, double *desc, bool want_desc)
{
    ModeSlot v[K];
#pragma unroll
    for (int j = 0; j < K; ++j) {
        v[j].m = th[1 + j];
        v[j].lt = th[1 + K + j];
        v[j].c = th[1 + 2 * K + j];
        v[j].key = key_group == MODE_KEY_M ? v[j].m : key_group == MODE_KEY_C ? v[j].c : v[j].lt;
        v[j].src = j;
    }
    mode_sort_network<K>(v);
    bool moved = false;
    ordered[0] = th[0];
#pragma unroll
    for (int j = 0; j < K; ++j) {
        ordered[1 + j] = v[j].m;
        ordered[1 + K + j] = v[j].lt;
        ordered[1 + 2 * K + j] = v[j].c;
        moved = moved || v[j].src != j;
    }
    if (want_desc) {
        double total = v[0].m;
#pragma unroll
        for (int j = 1; j < K; ++j) total = total + v[j].m;
        desc[0] = total;
#pragma unroll
        for (int j = 0; j < K; ++j) {
            const double l = log1p(-v[j].m);
            desc[1 + j] = v[j].lt + l / v[j].c;
            desc[1 + K + j] = v[j].lt + l / (2.0 * v[j].c);
        }
    }
    return moved;
}

// every row of every sample on the host: the arguments of bisip_mode_order_dev, host pointers; an output that is not
// asked for is a null pointer
template <int K>
inline void mode_order_rows_host(const double *chain, int64_t n_samples, int64_t sample_stride, int64_t rows, int key_group,
                                 double *ordered, double *desc, unsigned char *moved)
{
    constexpr int ND = 1 + 3 * K, NDESC = 1 + 2 * K;
    for (int64_t s = 0; s < n_samples; ++s)
        for (int64_t r = 0; r < rows; ++r) {
            double o[ND], d[NDESC];
            const bool mv = mode_order_row<K>(chain + s * sample_stride + r * ND, key_group, o, d, desc != nullptr);
            const int64_t at = s * rows + r;
            if (ordered)
                for (int k = 0; k < ND; ++k) ordered[at * ND + k] = o[k];
            if (desc)
                for (int k = 0; k < NDESC; ++k) desc[at * NDESC + k] = d[k];
            if (moved) moved[at] = mv ? 1 : 0;
        }
}

}  // namespace bisip
