// move_kernels.h -- the differential-evolution move (ter Braak 2006; emcee's DEMove) and the snooker move
// (ter Braak & Vrugt 2008; emcee's DESnookerMove) beside the stretch move of sampler_kernels.h, on the
// launch-per-half-step path: one launch per half-step, the LP::L lanes of a slot forming the same proposal and
// sharing its log-probability exactly as in k_stretch_half.  The red/blue halves and the active walker of slot t
// are the stretch contract's; partners are members of the complementary half.  bisip_amd/moves.py states the
// moves and their stream in NumPy, and every kernel here is held to it bit for bit.
//
//   DE       q_k = s_k + gamma * (ca_k - cb_k)                    factor = 0
//   snooker  d = s - z, n2 = sum d_k^2, u = d / sqrt(n2), p1 = sum u_k z1_k, p2 = sum u_k z2_k,
//            q_k = s_k + u_k * (gammas * (p1 - p2)), m2 = sum (q_k - z_k)^2
//            factor = 0.5 (ndim - 1) (ln m2 - ln n2);   n2 == 0: rejected, no flag
//   accept   (factor + logp(q)) - logp(s) > ln u
// Every sum runs k = 0 .. ndim-1, multiply then add: the library is built without contraction, so the roundings
// are the ones written here.
//
// The stream extends the Philox contract at DrawArgs (sampler_kernels.h): same key, the counter's fourth word
// names the purpose; purposes 0, 1 and 2 are untouched.
//   purpose 3, counter (k, 0, 0, 3):          the iteration's move, drawn on the host (moves.py: move_schedule)
//   purpose 4, counter (t, k, h | e << 1, 4): ranks in the other half (Nc members):
//                                             i0 = (x0 Nc) >> 32;  i1 = (x1 (Nc-1)) >> 32, +1 if >= i0;
//                                             i2 = (x2 (Nc-2)) >> 32, +1 if >= min(i0, i1), then +1 if >= max(i0, i1)
//                                             rank r is walker perm_inverse(2 r + 1 - h).  DE: a, b = i0, i1;
//                                             snooker: z, z1, z2 = i0, i1, i2
//   purpose 5, counter (t, k, h | e << 1, 5): n = sqrt(-2 ln(1 - u53(x0, x1))) cos(2 pi u53(x2, x3));
//                                             gamma = g0 (1 + sigma n)
//   ln u: the purpose-1 number of the slot, as a stretch iteration would have used it.
#pragma once
#include "sampler_kernels.h"

namespace bisip {

enum MoveKind { MOVE_STRETCH = 0, MOVE_DE = 1, MOVE_SNOOKER = 2 };

// a half-step of a move: the state, the slot's walker (s.active), its first partner (s.partner), ln u (s.logu) and
// where the rows go are the stretch launch's fields; s.zz and s.factor are not read
struct MoveArgs {
    StretchArgs s;
    const int *p1, *p2;      // (n_slots,) second and third partner (p2: snooker only)
    const double *gamma;     // (n_slots,) DE: g0 (1 + sigma n)
    double gammas;           // snooker: the scale of the jump
};

// proposal + log-prob + accept for slot t; all LP::L lanes of the slot run it
template <int MOVE, class LP>
__device__ __forceinline__ bool move_slot(const MoveArgs &a, const LP &lp, long long t, int g, int &walker,
                                          double (&row)[LP::NDIM], double &lp_row)
{
    constexpr int NDIM = LP::NDIM;
    static_assert(MOVE == MOVE_DE || MOVE == MOVE_SNOOKER, "the stretch move has kernels of its own");
    const int i = a.s.active[t];
    walker = i;
    const double *s_row = a.s.coords + (long long)i * NDIM;
    const double *c0 = a.s.coords + (long long)a.s.partner[t] * NDIM;
    const double *c1 = a.s.coords + (long long)a.p1[t] * NDIM;
    const double old_lp = a.s.logp[i];
    double s[NDIM], q[NDIM];
#pragma unroll
    for (int k = 0; k < NDIM; ++k) s[k] = s_row[k];
    double factor = 0.0;
    bool formed = true;
    if constexpr (MOVE == MOVE_DE) {
        const double gamma = a.gamma[t];
#pragma unroll
        for (int k = 0; k < NDIM; ++k) {
            const double d = c0[k] - c1[k];
            q[k] = s[k] + gamma * d;
        }
    } else {
        // z = c0; z1 and z2 are streamed into the two dot products: no rows of them are kept
        const double *c2 = a.s.coords + (long long)a.p2[t] * NDIM;
        double u[NDIM], n2 = 0.0;
#pragma unroll
        for (int k = 0; k < NDIM; ++k) {
            u[k] = s[k] - c0[k];
            n2 = n2 + u[k] * u[k];
        }
        const double norm = sqrt(n2);
        double p1 = 0.0, p2 = 0.0;
#pragma unroll
        for (int k = 0; k < NDIM; ++k) {
            u[k] = u[k] / norm;
            p1 = p1 + u[k] * c1[k];
            p2 = p2 + u[k] * c2[k];
        }
        const double jump = a.gammas * (p1 - p2);
        double m2 = 0.0;
#pragma unroll
        for (int k = 0; k < NDIM; ++k) {
            q[k] = s[k] + u[k] * jump;
            const double e = q[k] - c0[k];
            m2 = m2 + e * e;
        }
        factor = (0.5 * (NDIM - 1)) * (log(m2) - log(n2));
        // the walker sits on z: no direction.  Rejected; the lanes still evaluate (at s, so that the wavefront
        // exchanges of L > 1 stay whole) and no flag is raised
        formed = n2 != 0.0;
        if (!formed) {
#pragma unroll
            for (int k = 0; k < NDIM; ++k) q[k] = s[k];
            factor = 0.0;
        }
    }
    const double new_lp = lp(q, i, g);
    if (new_lp != new_lp) atomicOr(a.s.status, 1);
    const bool acc = formed && (factor + new_lp) - old_lp > a.s.logu[t];
#pragma unroll
    for (int k = 0; k < NDIM; ++k) row[k] = acc ? q[k] : s[k];
    lp_row = acc ? new_lp : old_lp;
    return acc;
}

// the half-step: k_stretch_half's shape, slot for slot (lanes past the last slot run clamped to it and never commit;
// every lane of a wave reads its rows before any lane commits, and no other wave touches them -- the partners of a
// half-step are never active in it)
template <class LP, int MOVE, int BLK = 64>
__global__ __launch_bounds__(BLK) void k_move_half(const MoveArgs a, const LP lp)
{
    constexpr int L = LP::L;
    const long long tid = (long long)blockIdx.x * BLK + threadIdx.x;
    const long long slot = tid / L;
    const int g = (int)(tid % L);
    const bool live = slot < a.s.n_slots;
    const long long t = live ? slot : a.s.n_slots - 1;
    int i;
    double row[LP::NDIM], lp_row;
    const bool acc = move_slot<MOVE>(a, lp, t, g, i, row, lp_row);
    if (live && g == 0) commit_row<LP::NDIM>(a.s, i, row, lp_row, acc);
}

// ---------------------------------------------------------------------------------
// the stream arrays of purposes 4, 5 and 1: (n_steps, 2, E, nh) as k_stretch_draw lays them out, global walker ids
// ---------------------------------------------------------------------------------
struct MoveDrawArgs {
    DrawHead s;
    double g0, sigma;                 // DE: gamma = g0 (1 + sigma n)
    int *active, *p0, *p1, *p2;
    double *gamma, *logu;
};

static __global__ __launch_bounds__(256) void k_move_draw(const MoveDrawArgs d)
{
    DrawSlot q;
    const DrawSlotKind kind = draw_decode(d.s, q);
    if (kind == DRAW_OUTSIDE) return;
    const long long k = q.k, e = q.e, t = q.t, idx = q.idx, W = d.s.W;
    const int h = q.h;
    if (kind == DRAW_PADDING) {
        d.active[idx] = 0; d.p0[idx] = 0; d.p1[idx] = 0; d.p2[idx] = 0; d.gamma[idx] = 0.0; d.logu[idx] = 0.0;
        return;
    }
    const unsigned step = (unsigned)(d.s.step0 + k), c2 = (unsigned)h | ((unsigned)(d.s.e0 + e) << 1);
    const long long Ns = h ? W / 2 : (W + 1) / 2, Nc = W - Ns;
    const long long Ainv = d.s.perm[3 * k + 1], B = d.s.perm[3 * k + 2];
    const Philox4 r1 = philox4x32_10((unsigned)t, step, c2, 1u, d.s.seed_lo, d.s.seed_hi);
    const Philox4 r4 = philox4x32_10((unsigned)t, step, c2, 4u, d.s.seed_lo, d.s.seed_hi);
    const Philox4 r5 = philox4x32_10((unsigned)t, step, c2, 5u, d.s.seed_lo, d.s.seed_hi);
    const long long i0 = (long long)(((unsigned long long)r4.v[0] * (unsigned long long)Nc) >> 32);
    long long i1 = (long long)(((unsigned long long)r4.v[1] * (unsigned long long)(Nc - 1)) >> 32);
    if (i1 >= i0) ++i1;
    const int base = (int)(e * W);
    d.active[idx] = base + perm_inverse(2 * t + h, W, Ainv, B);
    d.p0[idx] = base + perm_inverse(2 * i0 + (1 - h), W, Ainv, B);
    d.p1[idx] = base + perm_inverse(2 * i1 + (1 - h), W, Ainv, B);
    int third = 0;                          // a half of two has no third member: the field is 0
    if (Nc >= 3) {
        long long i2 = (long long)(((unsigned long long)r4.v[2] * (unsigned long long)(Nc - 2)) >> 32);
        if (i2 >= (i0 < i1 ? i0 : i1)) ++i2;
        if (i2 >= (i0 < i1 ? i1 : i0)) ++i2;
        third = base + perm_inverse(2 * i2 + (1 - h), W, Ainv, B);
    }
    d.p2[idx] = third;
    const double n = sqrt(-2.0 * log(1.0 - u53(r5.v[0], r5.v[1]))) * cos(6.283185307179586 * u53(r5.v[2], r5.v[3]));
    d.gamma[idx] = d.g0 * (1.0 + d.sigma * n);
    d.logu[idx] = log(u53(r1.v[0], r1.v[1]));
}

}  // namespace bisip
