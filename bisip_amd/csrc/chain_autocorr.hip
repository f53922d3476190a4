// chain_autocorr.hip -- integrated autocorrelation time of a device-resident chain
// (bisip_chain_autocorr_time_dev): emcee's integrated_time (emcee/autocorr.py, 3.1) for every
// (ensemble, parameter) of a chain that lives in HBM.
//
// For a chain x (n_t, E*Wp, ndim), every series j = (e*Wp + w)*ndim + d is centred and its
// autocorrelation acf_k = sum_{t < n_t-k} y_t y_{t+k} is taken as direct lag sums (emcee gets the same
// quantity from a zero-padded FFT), normalised by acf_0; f_k is the mean of the normalised acf over the
// walkers of an ensemble, taus = 2 cumsum(f) - 1 (sequential, as np.cumsum), and the window is the first
// lag where k < c*taus_k turns false (emcee's auto_window).  Three kernels:
//   1. k_ac_prep: mean and acf_0 of every series; one workgroup per tile of 64 series, the samples split
//      over its 16 waves and the partial sums added in a fixed order;
//   2. k_ac_lags: a round of L lags on the lag-sum tile of chain_lags.h; writes acf_k / acf_0 for the round's
//      lags into the workspace (L per series);
//   3. k_ac_walker_sums + k_ac_window: the round's normalised lags summed over the walkers of every
//      (ensemble, parameter) -- lanes over lags, groups of 256 walkers in order, then the groups in order --
//      and one wave per (ensemble, parameter) continues the cumulative sum and tests the window.
// Rounds are enqueued without a host synchronisation.  An (e, d) whose window is found is marked done;
// tiles whose series are all done leave the later rounds at once.  No floating-point atomics: the same
// chain gives the same bits every call.
#include "chain_lags.h"

using namespace bisip;
using namespace bisip::host;

namespace {

struct AcArgs {
    const double *chain;
    long long n_t, stride, E, Wp, M;   // M = E*Wp*ndim series
    int ndim;
    double c;
    long long L, k0;                   // lags per round, first lag of this round
    const double *mean, *a0;           // (M,)
    double *R;                         // (M, L): acf_k / acf_0 of the round
    double *cs;                        // (E*ndim,) cumulative sum of f so far
    long long *win;                    // (E*ndim,) window, -1 while not found
    double *tau;                       // (E*ndim,)
    long long *window_out;             // (E*ndim,) or null
};

__global__ __launch_bounds__(256) void k_ac_init(const AcArgs a)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.E * a.ndim) return;
    a.cs[i] = 0.0;
    a.win[i] = -1;
}

// mean and sum of centred squares of 64 series; wave q takes samples q, q + 16, ...
__global__ __launch_bounds__(LAG_PREP_WAVES * 64) void k_ac_prep(const AcArgs a, double *mean, double *a0)
{
    __shared__ double part[LAG_PREP_WAVES][LAG_TILE];
    __shared__ double mu[LAG_TILE];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long j = (long long)blockIdx.x * LAG_TILE + lane;
    const bool live = j < a.M;
    const double *x = a.chain + (live ? j : 0);
    double s = 0.0;
    if (live)
        for (long long t = wave; t < a.n_t; t += LAG_PREP_WAVES) s += x[t * a.stride];
    part[wave][lane] = s;
    __syncthreads();
    if (wave == 0) {
        double tot = 0.0;
        for (int q = 0; q < LAG_PREP_WAVES; ++q) tot += part[q][lane];
        mu[lane] = tot / (double)a.n_t;
    }
    __syncthreads();
    const double m = mu[lane];
    s = 0.0;
    if (live)
        for (long long t = wave; t < a.n_t; t += LAG_PREP_WAVES) {
            const double y = x[t * a.stride] - m;
            s = fma(y, y, s);
        }
    part[wave][lane] = s;      // wave 0 read the first partial sums before the barrier above
    __syncthreads();
    if (wave == 0 && live) {
        double tot = 0.0;
        for (int q = 0; q < LAG_PREP_WAVES; ++q) tot += part[q][lane];
        mean[j] = m;
        a0[j] = tot;
    }
}

// One round's lags [k0, k0 + L) of 64 series: workgroup (tile, b) takes the lag sums of lags kb = k0 + 64 b ... kb + 63
// over the n_t samples on the tile of chain_lags.h (the loop is k_ess_lags' of chain_ess.hip) and stores them over acf_0.
__global__ __launch_bounds__(LAG_WAVES * 64) void k_ac_lags(const AcArgs a)
{
    __shared__ double A[LAG_T][LAG_TILE];
    __shared__ double B[LAG_T + LAG_BLOCK][LAG_TILE];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long kb = a.k0 + (long long)blockIdx.y * LAG_BLOCK;
    if (kb >= a.n_t) return;
    const long long j = (long long)blockIdx.x * LAG_TILE + lane;
    const bool live = j < a.M;
    // the tile leaves when every series in it belongs to an (e, d) whose window is known
    // (the same 64 lanes in every wave: the exit is uniform over the workgroup)
    bool open = false;
    if (live) {
        const long long e = j / (a.Wp * a.ndim);
        const int d = (int)(j % a.ndim);
        open = a.win[e * a.ndim + d] < 0;
    }
    if (!__any(open)) return;
    const double m = live ? a.mean[j] : 0.0;
    const double *x = a.chain + (live ? j : 0);
    auto y = [&](long long t) { return live && t < a.n_t ? x[t * a.stride] - m : 0.0; };

    double acc[LAGS_WAVE];
#pragma unroll
    for (int i = 0; i < LAGS_WAVE; ++i) acc[i] = 0.0;
    const long long t_end = a.n_t - kb;     // samples that still meet a partner at lag kb
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
    const double n0 = a.a0[j];
    double *out = a.R + j * a.L + (kb - a.k0) + LAGS_WAVE * wave;
#pragma unroll
    for (int i = 0; i < LAGS_WAVE; ++i) {
        const long long k = kb + LAGS_WAVE * wave + i;
        // emcee divides acf by acf[0]: lag 0 is 1 exactly (NaN for a constant series)
        if (k < a.n_t) out[i] = k == 0 ? n0 / n0 : acc[i] / n0;
    }
}

// Walker sums of the round's normalised lags, in groups of LAG_GROUP walkers: workgroup (ed, g) adds
// walkers [g*LAG_GROUP, ...) of (e, d) in order, one lane per lag, into part[(ed*G + g)*L + kk].
// (A large ensemble spreads its walkers over many workgroups; the window kernel adds the groups in order.)
__global__ __launch_bounds__(64) void k_ac_walker_sums(const AcArgs a, double *part, long long G)
{
    const long long ed = blockIdx.x, g = blockIdx.y;
    if (a.win[ed] >= 0) return;
    const long long e = ed / a.ndim;
    const int d = (int)(ed % a.ndim);
    const long long w0 = g * LAG_GROUP, w1 = w0 + LAG_GROUP < a.Wp ? w0 + LAG_GROUP : a.Wp;
    const double *col = a.R + ((e * a.Wp + w0) * a.ndim + d) * a.L;
    const long long step = (long long)a.ndim * a.L;
    const long long n_round = a.n_t - a.k0 < a.L ? a.n_t - a.k0 : a.L;
    for (long long kk = threadIdx.x; kk < n_round; kk += 64) {
        double s = 0.0;
        for (long long w = 0; w < w1 - w0; ++w) s += col[w * step + kk];
        part[(ed * G + g) * a.L + kk] = s;
    }
}

// One wave per (e, d): f_k of the round's lags (lane = lag, the walker groups added in order), then lane 0
// continues the sequential cumulative sum and tests emcee's window m_k = k < c * taus_k.
__global__ __launch_bounds__(64) void k_ac_window(const AcArgs a, const double *part, long long G)
{
    __shared__ double f[64];
    __shared__ int stop;
    const long long ed = blockIdx.x;
    if (a.win[ed] >= 0) return;
    const int lane = threadIdx.x;
    const long long n_round = a.n_t - a.k0 < a.L ? a.n_t - a.k0 : a.L;
    double cs = a.cs[ed];
    if (lane == 0) stop = 0;
    for (long long c0 = 0; c0 < n_round; c0 += 64) {
        const long long kk = c0 + lane;
        if (kk < n_round) {
            double s = 0.0;
            for (long long g = 0; g < G; ++g) s += part[(ed * G + g) * a.L + kk];
            f[lane] = s / (double)a.Wp;
        }
        __syncthreads();
        if (lane == 0) {
            const int n = n_round - c0 < 64 ? (int)(n_round - c0) : 64;
            for (int q = 0; q < n; ++q) {
                const long long k = a.k0 + c0 + q;
                cs += f[q];
                const double taus = 2.0 * cs - 1.0;
                long long w = -1;
                double tau = taus;
                if (k == 0 && taus != taus) {
                    // f_0 is NaN (a constant walker): every taus is NaN, no m_k is true, the window is n_t - 1
                    w = a.n_t - 1;
                } else if (!((double)k < a.c * taus)) {
                    w = k;                        // the first lag where m turns false (m_0 is true)
                } else if (k == a.n_t - 1) {
                    w = 0;                        // m true at every lag: argmin(m) = 0, taus_0 = 1
                    tau = 1.0;
                }
                if (w >= 0) {
                    a.win[ed] = w;
                    a.tau[ed] = tau;
                    if (a.window_out) a.window_out[ed] = w;
                    stop = 1;
                    break;
                }
            }
            a.cs[ed] = cs;
        }
        __syncthreads();
        if (stop) return;
    }
}

struct Layout {
    long long M, tiles, L;
    long long G;                       // walker groups
    size_t mean, a0, R, part, cs, win, total;
};

Layout layout(long long n_t, long long E, long long Wp, int ndim)
{
    Layout l{};
    l.M = E * Wp * ndim;
    l.tiles = (l.M + LAG_TILE - 1) / LAG_TILE;
    l.L = round_lags(n_t, l.tiles);
    const long long P = E * ndim;
    l.mean = 0;
    l.a0 = l.mean + align256((size_t)l.M * 8);
    l.R = l.a0 + align256((size_t)l.M * 8);
    l.G = (Wp + LAG_GROUP - 1) / LAG_GROUP;
    l.part = l.R + align256((size_t)l.M * (size_t)l.L * 8);
    l.cs = l.part + align256((size_t)P * (size_t)l.G * (size_t)l.L * 8);
    l.win = l.cs + align256((size_t)P * 8);
    l.total = l.win + align256((size_t)P * 8);
    return l;
}

// ndim, then the counts.  E: one window workgroup per (e, d); Wp: the tiles within one grid dimension and the walker
// groups within grid dimension y.  n is not capped.
int check_shape(const ChainShape &s, Voice v)
{
    BISIP_TRY(check_ndim(s.ndim, 1, v));
    BISIP_TRY(check_counts(s, NO_CAP, GRID_MAX / s.ndim, NO_CAP, v));
    return check_counts(s, NO_CAP, NO_CAP, std::min<int64_t>(GRID_MAX * LAG_TILE / (s.E * s.ndim), 65535LL * LAG_GROUP), v);
}

}  // namespace

extern "C" {

int64_t bisip_chain_autocorr_time_workspace(int64_t n_samples, int64_t n_ensembles, int64_t walkers_per_ensemble, int ndim)
{
    if (check_shape({n_samples, 0, n_ensembles, walkers_per_ensemble, ndim}, QUIET) != BISIP_OK) return 0;
    return (int64_t)layout(n_samples, n_ensembles, walkers_per_ensemble, ndim).total;
}

int bisip_chain_autocorr_time_dev(const double *d_chain, int64_t n_samples, int64_t sample_stride, int64_t n_ensembles,
                                  int64_t walkers_per_ensemble, int ndim, double c, double *d_tau, int64_t *d_window,
                                  void *d_work, void *stream)
{
    if (!d_chain || !d_tau || !d_work) return fail(BISIP_EINVAL, "null argument");
    const ChainShape s{n_samples, sample_stride, n_ensembles, walkers_per_ensemble, ndim};
    BISIP_TRY(check_shape(s, LOUD));
    BISIP_TRY(check_stride(s));
    if (!(c > 0.0) || !std::isfinite(c)) return fail(BISIP_EINVAL, "c=%g: the window factor must be finite and > 0", c);
    const Layout l = layout(n_samples, n_ensembles, walkers_per_ensemble, ndim);
    char *base = (char *)d_work;
    AcArgs a{};
    a.chain = d_chain; a.n_t = n_samples; a.stride = sample_stride;
    a.E = n_ensembles; a.Wp = walkers_per_ensemble; a.ndim = ndim; a.M = l.M;
    a.c = c; a.L = l.L; a.k0 = 0;
    a.mean = (const double *)(base + l.mean);
    a.a0 = (const double *)(base + l.a0);
    a.R = (double *)(base + l.R);
    a.cs = (double *)(base + l.cs);
    a.win = (long long *)(base + l.win);
    a.tau = d_tau;
    a.window_out = (long long *)d_window;
    const long long P = n_ensembles * ndim;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_ac_init, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_ac_prep, dim3((unsigned)l.tiles), dim3(LAG_PREP_WAVES * 64), 0, st, a,
                       (double *)(base + l.mean), (double *)(base + l.a0));
    HIP_TRY(hipGetLastError());
    for (long long k0 = 0; k0 < n_samples; k0 += l.L) {
        a.k0 = k0;
        const long long nb = round_blocks(n_samples, k0, l.L);
        hipLaunchKernelGGL(k_ac_lags, dim3((unsigned)l.tiles, (unsigned)nb), dim3(LAG_WAVES * 64), 0, st, a);
        double *part = (double *)(base + l.part);
        hipLaunchKernelGGL(k_ac_walker_sums, dim3((unsigned)P, (unsigned)l.G), dim3(64), 0, st, a, part, l.G);
        hipLaunchKernelGGL(k_ac_window, dim3((unsigned)P), dim3(64), 0, st, a, (const double *)part, l.G);
        HIP_TRY(hipGetLastError());
    }
    return BISIP_OK;
}

}  // extern "C"
