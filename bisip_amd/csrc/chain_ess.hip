// chain_ess.hip -- effective sample size of a device-resident chain (bisip_chain_ess_dev) and the rank-normalisation
// that its bulk form is taken of (bisip_chain_rank_normalize_dev; folded about a centre: ..._folded_dev).  bisip_amd/ess.py holds the definitions in NumPy
// (ess_of_chains, z_scale): the estimator of Vehtari, Gelman, Simpson, Carpenter and Buerkner (2021) as Stan and ArviZ
// compute it.
//
// A half is the whole series (splits = 1, L = n) or its first and last L = n / 2 samples (splits = 2; the middle sample of
// an odd n is in neither).  A column j in [0, C), C = E * Wp * ndim, is one (ensemble, walker, parameter); a series is
// (threshold v, half, column): the values of the half, or with thresholds the indicator x <= thr[v, e, d] ? 1 : 0, or
// with a centre (bisip_chain_ess_squares_dev) the square (x - c[e, d]) * (x - c[e, d]), applied on load.  A pair p = (v * E + e) * ndim + d owns the M = splits * Wp chains c = half * Wp + w.
//   1. k_ess_prep: mean of every series from sums shifted by its first sample (a constant chain has mean exactly its
//      value and centred samples exactly 0), its min and max (NaN when a value is not finite); one workgroup per tile of
//      64 series, the samples split over its 16 waves and the partial sums added in a fixed order;
//   2. k_ess_lags: a round of Lr lags on the lag-sum tile of chain_lags.h; the pairs (t, t + k) stay inside the half;
//      writes the raw lag sums of the round into the workspace (Lr per series);
//   3. k_ess_chain_sums: the round's lag sums added over the chains of every pair -- lanes over lags, groups of 256 chains
//      in order, the scan adds the groups in order;
//   4. k_ess_scan: one wave per pair.  In round 0 it reduces the chains' means (their variance, two passes), minima and
//      maxima and decides NaN (a value not finite, a NaN threshold) and S (max - min < 1e-15).  Then lane 0 continues
//      Geyer's initial positive sequence over the round's lags.  The initial monotone sequence and tau need the
//      sequence only pair by pair, so they are taken on the way: a pair of rho is confirmed (capped by the running pair
//      sum, added to the sum) when the next one is consumed, and no rho is stored.  When the sequence ends the pair is
//      marked done; tiles whose pairs are all done leave the later rounds at once.
// Rounds are enqueued without a host synchronisation.  No floating-point atomics: the same chain gives the same bits
// every call.
#include "chain_lags.h"

using namespace bisip;
using namespace bisip::host;

namespace {

constexpr int ES_CHUNK = 256;                           // lags the scan stages in LDS at a time (even)
constexpr int ESS_MAX_THRESHOLDS = 8;
constexpr int ES_STATE = 8;        // doubles of scan state per pair

struct EssArgs {
    const double *chain;
    long long n, stride, E, Wp, C;     // C = E*Wp*ndim columns
    long long L, start1;               // samples of a half, first sample of half 1
    int ndim, splits, nthr;            // nthr >= 1 series sets (thr null: the values themselves)
    int mode;                          // ES_VALUES, ES_INDICATOR or ES_SQUARES
    const double *thr;                 // (nthr, E, ndim) thresholds, (E, ndim) centres (nthr = 1) or null
    long long Lr, k0;                  // lags per round, first lag of this round
    double *mean, *cmin, *cmax;        // (nthr*splits*C,) per series
    double *R;                         // (nthr*splits*C, Lr): raw lag sums of the round
    double *part;                      // (P, G, Lr): the chain groups' sums
    long long G;
    double *state;                     // (P, ES_STATE): even, odd, qa, qb, acc, mean_var, var_plus, var_means
    long long *t;                      // (P,)
    int *done;                         // (P,)
    double *ess;                       // (nthr, E, ndim)
};

// the series on load: the value, the indicator of a threshold, or the square about a centre -- one subtraction and one
// multiplication, each rounded (nothing is contracted: -ffp-contract=off)
enum { ES_VALUES = 0, ES_INDICATOR = 1, ES_SQUARES = 2 };

__device__ __forceinline__ double es_value(double x, int mode, double thr)
{
    if (mode == ES_INDICATOR) return x <= thr ? 1.0 : 0.0;
    if (mode == ES_SQUARES) {
        const double d = x - thr;
        return d * d;
    }
    return x;
}

// series z * C + j of chain c of pair (v, e, d)
__device__ __forceinline__ long long es_series(const EssArgs &a, long long v, long long e, int d, long long c)
{
    const long long half = c / a.Wp, w = c - half * a.Wp;
    return (v * a.splits + half) * a.C + (e * a.Wp + w) * a.ndim + d;
}

__global__ __launch_bounds__(256) void k_ess_init(const EssArgs a)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < (long long)a.nthr * a.E * a.ndim) a.done[i] = 0;
}

// mean, min and max of 64 series; wave q takes samples q, q + 16, ... of the half.  grid (tiles, nthr * splits)
__global__ __launch_bounds__(LAG_PREP_WAVES * 64) void k_ess_prep(const EssArgs a)
{
    __shared__ double ps[LAG_PREP_WAVES][LAG_TILE], plo[LAG_PREP_WAVES][LAG_TILE], phi[LAG_PREP_WAVES][LAG_TILE];
    __shared__ int pbad[LAG_PREP_WAVES][LAG_TILE];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long j = (long long)blockIdx.x * LAG_TILE + lane;
    const long long z = blockIdx.y, v = z / a.splits, half = z - v * a.splits;
    const bool live = j < a.C;
    const int mode = a.mode;
    double thr = 0.0, c = 0.0, s = 0.0, lo = __builtin_inf(), hi = -__builtin_inf();
    int bad = 0;
    if (live) {
        const long long e = j / (a.Wp * a.ndim);
        const int d = (int)(j % a.ndim);
        if (mode) thr = a.thr[(v * a.E + e) * a.ndim + d];
        const double *x = a.chain + (half ? a.start1 : 0) * a.stride + j;
        c = es_value(x[0], mode, thr);
        for (long long t = wave; t < a.L; t += LAG_PREP_WAVES) {
            const double val = es_value(x[t * a.stride], mode, thr);
            s += val - c;
            lo = fmin(lo, val);
            hi = fmax(hi, val);
            bad |= !__builtin_isfinite(val);
        }
    }
    ps[wave][lane] = s; plo[wave][lane] = lo; phi[wave][lane] = hi; pbad[wave][lane] = bad;
    __syncthreads();
    if (wave == 0 && live) {
        double tot = 0.0;
        for (int q = 0; q < LAG_PREP_WAVES; ++q) {
            tot += ps[q][lane];
            lo = fmin(lo, plo[q][lane]);
            hi = fmax(hi, phi[q][lane]);
            bad |= pbad[q][lane];
        }
        const long long at = z * a.C + j;
        a.mean[at] = c + tot / (double)a.L;
        a.cmin[at] = bad ? __builtin_nan("") : lo;
        a.cmax[at] = bad ? __builtin_nan("") : hi;
    }
}

// One round's lags [k0, k0 + Lr) of 64 series of one (threshold, half): grid (tiles, lag blocks, nthr * splits).
// Workgroup (tile, b) takes the lag sums of lags kb = k0 + 64 b ... kb + 63 over the L samples of the half on the tile of
// chain_lags.h (the loop is k_ac_lags' of chain_autocorr.hip) and stores them as they are.
__global__ __launch_bounds__(LAG_WAVES * 64) void k_ess_lags(const EssArgs a)
{
    __shared__ double A[LAG_T][LAG_TILE];
    __shared__ double B[LAG_T + LAG_BLOCK][LAG_TILE];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long kb = a.k0 + (long long)blockIdx.y * LAG_BLOCK;
    if (kb >= a.L) return;
    const long long j = (long long)blockIdx.x * LAG_TILE + lane;
    const long long z = blockIdx.z, v = z / a.splits, half = z - v * a.splits;
    const bool live = j < a.C;
    const int mode = a.mode;
    // the tile leaves when every series in it belongs to a pair whose sequence has ended
    // (the same 64 lanes in every wave: the exit is uniform over the workgroup)
    bool open = false;
    double thr = 0.0;
    if (live) {
        const long long e = j / (a.Wp * a.ndim);
        const int d = (int)(j % a.ndim);
        const long long p = (v * a.E + e) * a.ndim + d;
        open = a.done[p] == 0;
        if (mode) thr = a.thr[p];
    }
    if (!__any(open)) return;
    const double m = live ? a.mean[z * a.C + j] : 0.0;
    const double *x = a.chain + (half ? a.start1 : 0) * a.stride + (live ? j : 0);
    auto y = [&](long long t) { return live && t < a.L ? es_value(x[t * a.stride], mode, thr) - m : 0.0; };

    double acc[LAGS_WAVE];
#pragma unroll
    for (int i = 0; i < LAGS_WAVE; ++i) acc[i] = 0.0;
    const long long t_end = a.L - kb;       // samples that still meet a partner at lag kb
    for (long long t0 = 0; t0 < t_end; t0 += LAG_T) {
        __syncthreads();                    // the previous pass has read A and B
        for (int r = wave; r < LAG_T; r += LAG_WAVES) A[r][lane] = y(t0 + r);
        for (int r = wave; r < LAG_T + LAG_BLOCK; r += LAG_WAVES) B[r][lane] = y(t0 + kb + r);
        __syncthreads();
#pragma unroll
        for (int sc = 0; sc < LAG_T; sc += LAGS_WAVE) {
            double av[LAGS_WAVE], bv[2 * LAGS_WAVE];
#pragma unroll
            for (int s = 0; s < LAGS_WAVE; ++s) av[s] = A[sc + s][lane];
#pragma unroll
            for (int q = 0; q < 2 * LAGS_WAVE; ++q) bv[q] = B[sc + LAGS_WAVE * wave + q][lane];
#pragma unroll
            for (int s = 0; s < LAGS_WAVE; ++s)
#pragma unroll
                for (int i = 0; i < LAGS_WAVE; ++i) acc[i] = fma(av[s], bv[s + i], acc[i]);
        }
    }
    if (!live) return;
    double *out = a.R + (z * a.C + j) * a.Lr + (kb - a.k0) + LAGS_WAVE * wave;
#pragma unroll
    for (int i = 0; i < LAGS_WAVE; ++i)
        if (kb + LAGS_WAVE * wave + i < a.L) out[i] = acc[i];
}

// Chain sums of the round's lags, in groups of LAG_GROUP chains: workgroup (p, g) adds chains [g * 256, ...) of
// pair p in order, one lane per lag, into part[(p * G + g) * Lr + kk].
__global__ __launch_bounds__(64) void k_ess_chain_sums(const EssArgs a)
{
    const long long p = blockIdx.x, g = blockIdx.y;
    if (a.done[p]) return;
    const long long per = a.E * a.ndim, v = p / per, ed = p - v * per, e = ed / a.ndim;
    const int d = (int)(ed % a.ndim);
    const long long M = a.splits * a.Wp;
    const long long c0 = g * LAG_GROUP, c1 = c0 + LAG_GROUP < M ? c0 + LAG_GROUP : M;
    const long long n_round = a.L - a.k0 < a.Lr ? a.L - a.k0 : a.Lr;
    for (long long kk = threadIdx.x; kk < n_round; kk += 64) {
        double s = 0.0;
        for (long long c = c0; c < c1; ++c) s += a.R[es_series(a, v, e, d, c) * a.Lr + kk];
        a.part[(p * a.G + g) * a.Lr + kk] = s;
    }
}

// One wave per pair: abar_k of the round's lags (lane = lag, the chain groups added in order) staged in LDS, then lane 0
// continues the sequence.  even, odd: the pair of rho consumed last (rho[t - 1], rho[t]), not yet confirmed; qa, qb: the
// pair confirmed last, after its cap; acc: the sum of every confirmed rho.
__global__ __launch_bounds__(64) void k_ess_scan(const EssArgs a)
{
    __shared__ double f[ES_CHUNK];
    __shared__ int stop;
    const long long p = blockIdx.x;
    if (a.done[p]) return;
    const int lane = threadIdx.x;
    const long long per = a.E * a.ndim, v = p / per, ed = p - v * per, e = ed / a.ndim;
    const int d = (int)(ed % a.ndim);
    const long long M = a.splits * a.Wp, L = a.L;
    const double S = (double)L * (double)M;
    const long long n_round = L - a.k0 < a.Lr ? L - a.k0 : a.Lr;
    double *st = a.state + p * ES_STATE;
    double var_means = 0.0;
    if (a.k0 == 0) {
        double sum = 0.0, lo = __builtin_inf(), hi = -__builtin_inf();
        int bad = 0;
        for (long long c = lane; c < M; c += 64) {
            const long long s = es_series(a, v, e, d, c);
            const double cl = a.cmin[s], ch = a.cmax[s];
            sum += a.mean[s];
            bad |= cl != cl;
            lo = fmin(lo, cl);
            hi = fmax(hi, ch);
        }
        sum = wave_sum(sum);
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) {
            lo = fmin(lo, __shfl_xor(lo, s, 64));
            hi = fmax(hi, __shfl_xor(hi, s, 64));
        }
        bad = __any(bad) ? 1 : 0;
        if (a.thr) { const double thr = a.thr[p]; bad |= thr != thr; }
        const double mm = sum / (double)M;
        double t2 = 0.0;
        for (long long c = lane; c < M; c += 64) {
            const double dm = a.mean[es_series(a, v, e, d, c)] - mm;
            t2 = fma(dm, dm, t2);
        }
        t2 = wave_sum(t2);
        if (M > 1) var_means = t2 / (double)(M - 1);
        // (every lane holds the same bad, lo and hi: the exits are uniform)
        if (bad || hi - lo < 1e-15) {
            if (lane == 0) {
                a.ess[p] = bad ? __builtin_nan("") : S;
                a.done[p] = 1;
            }
            return;
        }
    }
    double even = 0.0, odd = 0.0, qa = 0.0, qb = 0.0, acc = 0.0, mean_var = 0.0, var_plus = 1.0;
    long long t = 1;
    if (lane == 0) {
        stop = 0;
        if (a.k0 > 0) {
            even = st[0]; odd = st[1]; qa = st[2]; qb = st[3]; acc = st[4]; mean_var = st[5]; var_plus = st[6];
            t = a.t[p];
        }
    }
    for (long long c0 = 0; c0 < n_round; c0 += ES_CHUNK) {
        __syncthreads();                              // lane 0 has read the previous chunk (and stop is set)
        const int nc = n_round - c0 < ES_CHUNK ? (int)(n_round - c0) : ES_CHUNK;
        for (int i = lane; i < nc; i += 64) {
            double s = 0.0;
            for (long long g = 0; g < a.G; ++g) s += a.part[(p * a.G + g) * a.Lr + c0 + i];
            f[i] = s / (double)L / (double)M;
        }
        __syncthreads();
        if (lane == 0) {
            const long long base = a.k0 + c0;         // the lag of f[0]: even
            if (base == 0) {                          // (L >= 2: f[1] is there)
                mean_var = f[0] * (double)L / (double)(L - 1);
                var_plus = f[0] + var_means;
                even = 1.0;
                odd = 1.0 - (mean_var - f[1]) / var_plus;
                qa = qb = __builtin_inf();            // nothing confirmed yet: no cap
                acc = 0.0;
                t = 1;
            }
            for (;;) {
                if (!(t < L - 3 && even + odd > 0.0)) {
                    // the sequence ends: max_t = t - 2, every rho up to there is confirmed; rho[max_t + 1] is even when
                    // that is positive, else what was stored: even when the last pair summed to >= 0, else 0
                    const double last = even > 0.0 ? even : (even + odd >= 0.0 ? even : 0.0);
                    double tau = -1.0 + 2.0 * acc + last;
                    const double floor_tau = 1.0 / log10(S);
                    if (!(tau >= floor_tau)) tau = floor_tau;
                    a.ess[p] = S / tau;
                    a.done[p] = 1;
                    stop = 1;
                    break;
                }
                const long long k = t + 1;            // even, >= base
                if (k + 1 >= base + nc) break;        // the next pair lies in a later chunk or round
                double pa = even, pb = odd;           // confirm the pair consumed last: the initial monotone sequence
                if (pa + pb > qa + qb) pa = pb = (qa + qb) / 2.0;
                acc += pa + pb;
                qa = pa; qb = pb;
                even = 1.0 - (mean_var - f[k - base]) / var_plus;
                odd = 1.0 - (mean_var - f[k + 1 - base]) / var_plus;
                t += 2;
            }
        }
        __syncthreads();
        if (stop) return;
    }
    if (lane == 0) {
        st[0] = even; st[1] = odd; st[2] = qa; st[3] = qb; st[4] = acc; st[5] = mean_var; st[6] = var_plus;
        a.t[p] = t;
    }
}

struct Layout {
    long long L, C, Z, P, M, G, Lr, tiles;
    size_t mean, cmin, cmax, R, part, state, t, done, total;
};

// ndim, the splits, the samples of a half, then the counts.  n: 32 bits; E: one scan workgroup per (threshold, ensemble,
// parameter) of ESS_MAX_THRESHOLDS thresholds; Wp: the tiles within grid dimension x and the chain groups of both halves
// within grid dimension y.  (The number of thresholds is the entry point's to check.)
int check_ess_shape(const ChainShape &s, int splits, Voice v)
{
    BISIP_TRY(check_ndim(s.ndim, 1, v));
    if (splits != 1 && splits != 2) return refuse(v, BISIP_EINVAL, "splits=%d: 1 or 2", splits);
    if (s.n < 2 * splits) return refuse(v, BISIP_EINVAL, "n_samples=%lld: a chain needs 2 samples, a half too", (long long)s.n);
    BISIP_TRY(check_counts(s, GRID_MAX, GRID_MAX / (s.ndim * ESS_MAX_THRESHOLDS), NO_CAP, v));
    return check_counts(s, NO_CAP, NO_CAP, std::min<int64_t>(GRID_MAX * LAG_TILE / (s.E * s.ndim), 65535LL * LAG_GROUP / 2), v);
}

Layout ess_layout(long long n, long long E, long long Wp, int ndim, int splits, int n_threshold)
{
    Layout l{};
    const long long nthr = n_threshold > 0 ? n_threshold : 1;
    l.L = splits == 2 ? n / 2 : n;
    l.C = E * Wp * ndim;
    l.Z = nthr * splits;
    l.P = nthr * E * ndim;
    l.M = splits * Wp;
    l.G = (l.M + LAG_GROUP - 1) / LAG_GROUP;
    l.tiles = (l.C + LAG_TILE - 1) / LAG_TILE;
    l.Lr = round_lags(l.L, l.tiles * l.Z);
    const size_t series = align256((size_t)l.Z * (size_t)l.C * 8);
    l.mean = 0;
    l.cmin = l.mean + series;
    l.cmax = l.cmin + series;
    l.R = l.cmax + series;
    l.part = l.R + align256((size_t)l.Z * (size_t)l.C * (size_t)l.Lr * 8);
    l.state = l.part + align256((size_t)l.P * (size_t)l.G * (size_t)l.Lr * 8);
    l.t = l.state + align256((size_t)l.P * ES_STATE * 8);
    l.done = l.t + align256((size_t)l.P * 8);
    l.total = l.done + align256((size_t)l.P * 4);
    return l;
}

// what bisip_chain_ess_dev and bisip_chain_ess_squares_dev share: the checks of the shape, the layout and the rounds.
// d_aux: the thresholds (n_threshold of them), the centres (n_threshold = 0) or null.
int ess_run(const double *d_chain, int64_t n_samples, int64_t sample_stride, int64_t n_ensembles,
            int64_t walkers_per_ensemble, int ndim, int splits, int mode, const double *d_aux, int n_threshold,
            double *d_ess, void *d_work, int64_t work_bytes, void *stream)
{
    const ChainShape s{n_samples, sample_stride, n_ensembles, walkers_per_ensemble, ndim};
    BISIP_TRY(check_ess_shape(s, splits, LOUD));
    BISIP_TRY(check_stride(s));
    const Layout l = ess_layout(n_samples, n_ensembles, walkers_per_ensemble, ndim, splits, n_threshold);
    BISIP_TRY(check_workspace(d_work, work_bytes, (int64_t)l.total));
    char *base = (char *)d_work;
    EssArgs a{};
    a.chain = d_chain; a.n = n_samples; a.stride = sample_stride; a.E = n_ensembles; a.Wp = walkers_per_ensemble;
    a.C = l.C; a.L = l.L; a.start1 = n_samples - l.L; a.ndim = ndim; a.splits = splits;
    a.nthr = n_threshold > 0 ? n_threshold : 1;
    a.mode = mode; a.thr = d_aux; a.Lr = l.Lr; a.k0 = 0;
    a.mean = (double *)(base + l.mean); a.cmin = (double *)(base + l.cmin); a.cmax = (double *)(base + l.cmax);
    a.R = (double *)(base + l.R); a.part = (double *)(base + l.part); a.G = l.G;
    a.state = (double *)(base + l.state); a.t = (long long *)(base + l.t); a.done = (int *)(base + l.done);
    a.ess = d_ess;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_ess_init, dim3((unsigned)((l.P + 255) / 256)), dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_ess_prep, dim3((unsigned)l.tiles, (unsigned)l.Z), dim3(LAG_PREP_WAVES * 64), 0, st, a);
    HIP_TRY(hipGetLastError());
    for (long long k0 = 0; k0 < l.L; k0 += l.Lr) {
        a.k0 = k0;
        const long long nb = round_blocks(l.L, k0, l.Lr);
        hipLaunchKernelGGL(k_ess_lags, dim3((unsigned)l.tiles, (unsigned)nb, (unsigned)l.Z), dim3(LAG_WAVES * 64), 0, st, a);
        hipLaunchKernelGGL(k_ess_chain_sums, dim3((unsigned)l.P, (unsigned)l.G), dim3(64), 0, st, a);
        hipLaunchKernelGGL(k_ess_scan, dim3((unsigned)l.P), dim3(64), 0, st, a);
        HIP_TRY(hipGetLastError());
    }
    return BISIP_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// rank-normalisation
// ---------------------------------------------------------------------------------------------------------------
// Wichura (1988), Algorithm AS 241, routine PPND16: the published coefficients, highest power first.  Multiplications
// and additions in the order of bisip_amd/ess.py (ndtri); nothing is contracted (-ffp-contract=off).
__device__ __forceinline__ double es_horner(const double (&c)[8], double r)
{
    double v = c[0] * r;
#pragma unroll
    for (int i = 1; i < 7; ++i) v = (v + c[i]) * r;
    return v + c[7];
}

__device__ double es_ppnd16(double p)
{
    constexpr double A[8] = {2.5090809287301226727e+3, 3.3430575583588128105e+4, 6.7265770927008700853e+4,
                             4.5921953931549871457e+4, 1.3731693765509461125e+4, 1.9715909503065514427e+3,
                             1.3314166789178437745e+2, 3.3871328727963666080e+0};
    constexpr double B[8] = {5.2264952788528545610e+3, 2.8729085735721942674e+4, 3.9307895800092710610e+4,
                             2.1213794301586595867e+4, 5.3941960214247511077e+3, 6.8718700749205790830e+2,
                             4.2313330701600911252e+1, 1.0};
    constexpr double C[8] = {7.74545014278341407640e-4, 2.27238449892691845833e-2, 2.41780725177450611770e-1,
                             1.27045825245236838258e+0, 3.64784832476320460504e+0, 5.76949722146069140550e+0,
                             4.63033784615654529590e+0, 1.42343711074968357734e+0};
    constexpr double D[8] = {1.05075007164441684324e-9, 5.47593808499534494600e-4, 1.51986665636164571966e-2,
                             1.48103976427480074590e-1, 6.89767334985100004550e-1, 1.67638483018380384940e+0,
                             2.05319162663775882187e+0, 1.0};
    constexpr double E[8] = {2.01033439929228813265e-7, 2.71155556874348757815e-5, 1.24266094738807843860e-3,
                             2.65321895265761230930e-2, 2.96560571828504891230e-1, 1.78482653991729133580e+0,
                             5.46378491116411436990e+0, 6.65790464350110377720e+0};
    constexpr double F[8] = {2.04426310338993978564e-15, 1.42151175831644588870e-7, 1.84631831751005468180e-5,
                             7.86869131145613259100e-4, 1.48753612908506148525e-2, 1.36929880922735805310e-1,
                             5.99832206555887937690e-1, 1.0};
    const double q = p - 0.5;
    if (fabs(q) <= 0.425) {
        const double r = 0.180625 - q * q;
        return es_horner(A, r) * q / es_horner(B, r);
    }
    double r = sqrt(-log(q <= 0.0 ? p : 1.0 - p));
    double x;
    if (r <= 5.0) {
        r -= 1.6;
        x = es_horner(C, r) / es_horner(D, r);
    } else {
        r -= 5.0;
        x = es_horner(E, r) / es_horner(F, r);
    }
    return q < 0.0 ? -x : x;
}

struct RankArgs {
    const double *chain;
    long long n, stride, E, Wp;
    int ndim;
    const double *sorted;      // (E*ndim, N): every column in ascending order
    long long N;               // n * Wp values of a column
    double *z;                 // (n, E*Wp, ndim)
    const double *center;      // (E, ndim): the ranks are those of fabs(x - center); null: of x itself
};

// The fold of bisip_chain_rank_normalize_folded_dev on the gathered columns, in place, before they are sorted: one
// thread per value, column e * ndim + q about center[e * ndim + q].  One IEEE subtraction and fabs, as in k_rank_z.
__global__ __launch_bounds__(256) void k_fold_columns(double *cols, long long N, long long items, const double *center)
{
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= items) return;
    cols[idx] = fabs(cols[idx] - center[idx / N]);
}

// One thread per chain element, in the order of the chain: both sides coalesced.  below = how many values of its sorted
// column are smaller, upto = how many are not larger (two binary searches: no index goes through the sort); its ties
// hold the ranks below + 1 ... upto, whose mean is (below + upto + 1) / 2.  The sort puts whatever is not finite at one
// of the two ends of the column.  With a centre the element is folded as its column was, by the same two operations.
__global__ __launch_bounds__(256) void k_rank_z(const RankArgs a)
{
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long row = a.E * a.Wp * a.ndim;
    if (idx >= a.n * row) return;
    const long long s = idx / row, rest = idx - s * row, r = rest / a.ndim, e = r / a.Wp;
    const int q = (int)(rest - r * a.ndim);
    const double *__restrict__ col = a.sorted + (e * a.ndim + q) * a.N;
    double x = a.chain[s * a.stride + rest];
    if (a.center) x = fabs(x - a.center[e * a.ndim + q]);
    double out = __builtin_nan("");
    if (__builtin_isfinite(col[0]) && __builtin_isfinite(col[a.N - 1])) {
        long long lo = 0, hi = a.N;
        while (lo < hi) {
            const long long mid = lo + ((hi - lo) >> 1);
            if (col[mid] < x) lo = mid + 1; else hi = mid;
        }
        const long long below = lo;
        hi = a.N;
        while (lo < hi) {
            const long long mid = lo + ((hi - lo) >> 1);
            if (col[mid] <= x) lo = mid + 1; else hi = mid;
        }
        const double rank = (double)(below + lo + 1) / 2.0;
        out = es_ppnd16((rank - 0.375) / ((double)a.N + 0.25));
    }
    a.z[idx] = out;
}

struct RankPlan {
    long long N, columns, items;
    size_t col_bytes, temp_bytes, need;
};

// ndim and the counts, none of which is capped as a bad shape: a chain beyond the 2^31 items of one sort is unsupported
int rank_plan(int64_t n, int64_t E, int64_t Wp, int ndim, RankPlan &p, Voice v)
{
    BISIP_TRY(check_ndim(ndim, 1, v));
    BISIP_TRY(check_counts({n, 0, E, Wp, ndim}, NO_CAP, NO_CAP, NO_CAP, v));
    if (n > GRID_MAX || E > GRID_MAX || Wp > GRID_MAX || (p.N = n * Wp) > GRID_MAX || (p.columns = E * ndim) > GRID_MAX ||
        p.N * p.columns > GRID_MAX)
        return refuse(v, BISIP_EUNSUPPORTED, "chain exceeds the 2^31 items of one sort");
    p.items = p.N * p.columns;
    p.col_bytes = align256((size_t)p.items * 8);
    p.temp_bytes = sort_scratch_bound(p.items, p.columns);
    p.need = 2 * p.col_bytes + align256(p.temp_bytes);
    return BISIP_OK;
}

// what bisip_chain_rank_normalize_dev (d_center null) and bisip_chain_rank_normalize_folded_dev share
int rank_run(const double *d_chain, int64_t n_samples, int64_t sample_stride, int64_t n_ensembles,
             int64_t walkers_per_ensemble, int ndim, const double *d_center, double *d_z, void *d_work, int64_t work_bytes,
             void *stream)
{
    RankPlan p{};
    BISIP_TRY(rank_plan(n_samples, n_ensembles, walkers_per_ensemble, ndim, p, LOUD));
    BISIP_TRY(check_stride({n_samples, sample_stride, n_ensembles, walkers_per_ensemble, ndim}));
    BISIP_TRY(check_workspace(d_work, work_bytes, (int64_t)p.need));
    hipStream_t st = (hipStream_t)stream;
    char *base = (char *)d_work;
    double *cols = (double *)base, *sorted = (double *)(base + p.col_bytes);
    int rc = gather_columns(d_chain, n_samples, sample_stride, n_ensembles, walkers_per_ensemble, ndim, cols, st);
    if (rc != BISIP_OK) return rc;
    if (d_center) {
        hipLaunchKernelGGL(k_fold_columns, dim3((unsigned)((p.items + 255) / 256)), dim3(256), 0, st, cols, p.N, p.items, d_center);
        HIP_TRY(hipGetLastError());
    }
    rc = sort_segments(base + 2 * p.col_bytes, p.temp_bytes, cols, sorted, p.items, p.columns, p.N, st);
    if (rc != BISIP_OK) return rc;
    const RankArgs ra{d_chain, n_samples, sample_stride, n_ensembles, walkers_per_ensemble, ndim, sorted, p.N, d_z, d_center};
    hipLaunchKernelGGL(k_rank_z, dim3((unsigned)((p.items + 255) / 256)), dim3(256), 0, st, ra);
    HIP_TRY(hipGetLastError());
    return BISIP_OK;
}

}  // namespace

extern "C" {

int64_t bisip_chain_ess_workspace(int64_t n_samples, int64_t n_ensembles, int64_t walkers_per_ensemble, int ndim, int splits,
                                  int n_threshold)
{
    if (n_threshold < 0 || n_threshold > ESS_MAX_THRESHOLDS) return 0;
    if (check_ess_shape({n_samples, 0, n_ensembles, walkers_per_ensemble, ndim}, splits, QUIET) != BISIP_OK) return 0;
    return (int64_t)ess_layout(n_samples, n_ensembles, walkers_per_ensemble, ndim, splits, n_threshold).total;
}

int bisip_chain_ess_dev(const double *d_chain, int64_t n_samples, int64_t sample_stride, int64_t n_ensembles,
                        int64_t walkers_per_ensemble, int ndim, int splits, const double *d_threshold, int n_threshold,
                        double *d_ess, void *d_work, int64_t work_bytes, void *stream)
{
    if (!d_chain || !d_ess || !d_work) return fail(BISIP_EINVAL, "null argument");
    if (d_threshold ? (n_threshold < 1 || n_threshold > ESS_MAX_THRESHOLDS) : n_threshold != 0)
        return fail(BISIP_EINVAL, "n_threshold=%d: 1 ... %d with thresholds, 0 without", n_threshold, ESS_MAX_THRESHOLDS);
    return ess_run(d_chain, n_samples, sample_stride, n_ensembles, walkers_per_ensemble, ndim, splits,
                   d_threshold ? ES_INDICATOR : ES_VALUES, d_threshold, n_threshold, d_ess, d_work, work_bytes, stream);
}

int bisip_chain_ess_squares_dev(const double *d_chain, int64_t n_samples, int64_t sample_stride, int64_t n_ensembles,
                                int64_t walkers_per_ensemble, int ndim, int splits, const double *d_center, double *d_ess,
                                void *d_work, int64_t work_bytes, void *stream)
{
    if (!d_chain || !d_center || !d_ess || !d_work) return fail(BISIP_EINVAL, "null argument");
    return ess_run(d_chain, n_samples, sample_stride, n_ensembles, walkers_per_ensemble, ndim, splits, ES_SQUARES, d_center, 0,
                   d_ess, d_work, work_bytes, stream);
}

int64_t bisip_chain_rank_normalize_workspace(int64_t n_samples, int64_t n_ensembles, int64_t walkers_per_ensemble, int ndim)
{
    RankPlan p{};
    if (rank_plan(n_samples, n_ensembles, walkers_per_ensemble, ndim, p, QUIET) != BISIP_OK) return 0;
    return (int64_t)p.need;
}

int bisip_chain_rank_normalize_dev(const double *d_chain, int64_t n_samples, int64_t sample_stride, int64_t n_ensembles,
                                   int64_t walkers_per_ensemble, int ndim, double *d_z, void *d_work, int64_t work_bytes,
                                   void *stream)
{
    if (!d_chain || !d_z || !d_work) return fail(BISIP_EINVAL, "null argument");
    return rank_run(d_chain, n_samples, sample_stride, n_ensembles, walkers_per_ensemble, ndim, nullptr, d_z, d_work,
                    work_bytes, stream);
}

int bisip_chain_rank_normalize_folded_dev(const double *d_chain, int64_t n_samples, int64_t sample_stride,
                                          int64_t n_ensembles, int64_t walkers_per_ensemble, int ndim,
                                          const double *d_center, double *d_z, void *d_work, int64_t work_bytes, void *stream)
{
    if (!d_chain || !d_center || !d_z || !d_work) return fail(BISIP_EINVAL, "null argument");
    return rank_run(d_chain, n_samples, sample_stride, n_ensembles, walkers_per_ensemble, ndim, d_center, d_z, d_work,
                    work_bytes, stream);
}

}  // extern "C"
