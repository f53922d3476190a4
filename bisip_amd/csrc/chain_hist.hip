// chain_hist.hip -- the shapes of the posterior of a device-resident chain: the range of every parameter, its histogram
// and the histogram of every pair (bisip_chain_range_dev, bisip_chain_histograms_dev, bisip_chain_pair_histograms_dev).
//
// The reference's plot_histograms (src/bisip/plotlib.py:56-90: np.histogram of every parameter) and plot_corner
// (:233-259: corner's 1-D and pairwise 2-D histograms) are counted here.
// The bin edges come from the host (np.linspace); value x is in bin i iff edges[i] <= x < edges[i+1], x == edges[bins]
// is in the last bin, everything else (outside, NaN) is counted nowhere: the comparisons against the uploaded edges
// decide, (x - lo) * bins / (hi - lo) is only the first guess.  These are np.histogram's / np.histogram2d's integers.
//   * A workgroup takes ensemble e, a range of samples and a range of walkers (chain_splits: enough workgroups to
//     fill the chip, fewer than 2^31 rows each), counts into uint32 LDS counters with LDS atomics and adds them to
//     the int64 result with global integer atomics: integer sums, the same bits in any order.
//   * k_chain_histograms / k_chain_range read like k_moments_partial: consecutive lanes read consecutive doubles, a
//     lane always sees the same parameter.  A lane adds a RUN of values that fall in the same bin with one atomic:
//     a narrow posterior inside wide edges (range = prior bounds) puts all values into one or two bins, and a
//     workgroup's lanes would otherwise take turns on one LDS word.
//   * k_pair_histograms: one thread per row; its ND bin indices are found once and used for all pairs.  When eight
//     or more lanes of a wave hit the cell of its first lane, one lane adds their number.  The pairs
//     (np.triu_indices order) go in groups of consecutive pairs whose bins x bins counters fit 64 KiB of LDS with
//     the edges: blockIdx.y is the group (ndim = 7, bins = 20: one group of 21; ndim = 16: four groups at
//     bins = 20, 40 at bins = 64).
#include "chain.h"
#include "select_key.h"

using namespace bisip;
using namespace bisip::host;

namespace {

constexpr size_t HIST_LDS_BYTES = 65536;

struct HistArgs {
    const double *chain;     // first used sample
    long long n_samples, sample_stride, E, Wp;
    long long ss, sw;        // sample ranges and walker ranges per ensemble (chain_splits)
    int ndim, bins;
    int group, npairs;       // pairs per workgroup, pairs in all (k_pair_histograms)
    const double *edges;     // (E, ndim, bins + 1)
    unsigned long long *counts;    // (E, ndim, bins) or (E, npairs, bins, bins)
    unsigned long long *keys;      // (E, ndim, 2) running min / max as ordered keys (k_chain_range)
    unsigned long long *nonfinite; // (E, ndim)
};

struct ChainSplit { long long ss, sw; };

// `wanted` workgroups over the chip: per ensemble ss ranges of samples (four samples each at least) times sw ranges of
// walkers (256 walkers each at least); more than that only to keep a workgroup's rows under 2^31
ChainSplit chain_splits(long long n, long long E, long long Wp, long long wanted)
{
    const long long per = (wanted + E - 1) / E;
    long long ss = n / 4 < per ? n / 4 : per;
    if (ss < 1) ss = 1;
    long long sw = (per + ss - 1) / ss;
    if (sw > Wp / 256) sw = Wp / 256;
    if (sw < 1) sw = 1;
    while (((n + ss - 1) / ss) * ((Wp + sw - 1) / sw) > 0x7fffffffLL) {
        if (ss < n) ss = 2 * ss < n ? 2 * ss : n;
        else sw = 2 * sw < Wp ? 2 * sw : Wp;
    }
    return ChainSplit{ss, sw};
}

// the part of the chain workgroup blockIdx.x owns: ensemble e, samples [s0, s1), walkers [w0, w1)
struct ChainPart { long long e, s0, s1, w0, w1; };

__device__ __forceinline__ ChainPart chain_part(const HistArgs &a)
{
    long long b = blockIdx.x;
    const long long tw = b % a.sw; b /= a.sw;
    const long long sp = b % a.ss, e = b / a.ss;
    return ChainPart{e, a.n_samples * sp / a.ss, a.n_samples * (sp + 1) / a.ss, a.Wp * tw / a.sw, a.Wp * (tw + 1) / a.sw};
}

// bin of x among ed[0 ... bins], -1 if none; lo = ed[0], hi = ed[bins], scale = bins / (hi - lo)
__device__ __forceinline__ int find_bin(const double *ed, int bins, double lo, double hi, double scale, double x)
{
    if (!(x >= lo && x <= hi)) return -1;                // outside, or NaN
    int i = (int)((x - lo) * scale);                     // (saturating conversion; NaN -> 0)
    i = i < 0 ? 0 : (i > bins - 1 ? bins - 1 : i);
    while (i > 0 && x < ed[i]) --i;
    while (i < bins - 1 && x >= ed[i + 1]) ++i;
    return i;
}

// f(x) for every value of this lane in the part: lane t of the first `lanes` = (256 / ndim) * ndim reads doubles
// t, t + lanes, ... of the walker range of each sample (always parameter t % ndim), four samples in flight
template <typename F>
__device__ __forceinline__ void for_each_value(const HistArgs &a, const ChainPart &p, int t, int lanes, F &&f)
{
    const long long i0 = p.w0 * a.ndim, i1 = p.w1 * a.ndim;
    const double *base = a.chain + p.e * a.Wp * a.ndim;
    long long s = p.s0;
    for (; s + 4 <= p.s1; s += 4) {
        const double *r = base + s * a.sample_stride;
        for (long long i = i0 + t; i < i1; i += lanes) {
            const double x0 = __builtin_nontemporal_load(r + i), x1 = __builtin_nontemporal_load(r + a.sample_stride + i);
            const double x2 = __builtin_nontemporal_load(r + 2 * a.sample_stride + i);
            const double x3 = __builtin_nontemporal_load(r + 3 * a.sample_stride + i);
            f(x0); f(x1); f(x2); f(x3);
        }
    }
    for (; s < p.s1; ++s) {
        const double *r = base + s * a.sample_stride;
        for (long long i = i0 + t; i < i1; i += lanes) f(__builtin_nontemporal_load(r + i));
    }
}

__global__ __launch_bounds__(256) void k_chain_range_init(const HistArgs a)
{
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;      // (e, q)
    if (idx >= a.E * a.ndim) return;
    a.keys[2 * idx] = ~0ull;
    a.keys[2 * idx + 1] = 0ull;
    a.nonfinite[idx] = 0ull;
}

// min and max of the finite values as ordered keys (integer min / max: any order gives the same bits), and the
// number of values that are not finite
__global__ __launch_bounds__(256) void k_chain_range(const HistArgs a)
{
    __shared__ unsigned long long smin[256], smax[256];
    __shared__ unsigned sbad[256];
    const int t = threadIdx.x, per = 256 / a.ndim, lanes = per * a.ndim;
    const ChainPart p = chain_part(a);
    unsigned long long kmin = ~0ull, kmax = 0ull;
    unsigned bad = 0;
    if (t < lanes)
        for_each_value(a, p, t, lanes, [&](double x) {
            const unsigned long long u = (unsigned long long)__double_as_longlong(x);
            if ((u & 0x7ff0000000000000ull) == 0x7ff0000000000000ull) { ++bad; return; }
            const unsigned long long k = select_key(x);
            kmin = k < kmin ? k : kmin;
            kmax = k > kmax ? k : kmax;
        });
    smin[t] = kmin; smax[t] = kmax; sbad[t] = bad;
    __syncthreads();
    if (t < a.ndim) {
        unsigned long long total = 0;
        for (int k = 0; k < per; ++k) {
            const int j = k * a.ndim + t;
            kmin = smin[j] < kmin ? smin[j] : kmin;
            kmax = smax[j] > kmax ? smax[j] : kmax;
            total += sbad[j];
        }
        const long long idx = p.e * a.ndim + t;
        if (kmin <= kmax) {                       // (a part without a finite value adds nothing)
            atomicMin(&a.keys[2 * idx], kmin);
            atomicMax(&a.keys[2 * idx + 1], kmax);
        }
        if (total) atomicAdd(&a.nonfinite[idx], total);
    }
}

// keys -> doubles, in place; a column without a finite value: (+inf, -inf)
__global__ __launch_bounds__(256) void k_chain_range_finish(const HistArgs a)
{
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;      // (e, q)
    if (idx >= a.E * a.ndim) return;
    const unsigned long long kmin = a.keys[2 * idx], kmax = a.keys[2 * idx + 1];
    double *out = (double *)a.keys;
    const bool none = kmin > kmax;
    out[2 * idx] = none ? __builtin_inf() : select_value(kmin);
    out[2 * idx + 1] = none ? -__builtin_inf() : select_value(kmax);
}

__global__ __launch_bounds__(256) void k_chain_histograms(const HistArgs a)
{
    extern __shared__ double s_hist[];
    const int nb = a.bins, ne = nb + 1;
    double *s_edges = s_hist;                                  // (ndim, bins + 1)
    unsigned *s_cnt = (unsigned *)(s_edges + a.ndim * ne);     // (ndim, bins)
    const int t = threadIdx.x, per = 256 / a.ndim, lanes = per * a.ndim;
    const ChainPart p = chain_part(a);
    const double *ge = a.edges + p.e * a.ndim * ne;
    for (int i = t; i < a.ndim * ne; i += 256) s_edges[i] = ge[i];
    for (int i = t; i < a.ndim * nb; i += 256) s_cnt[i] = 0u;
    __syncthreads();
    if (t < lanes) {
        const int q = t % a.ndim;
        const double *ed = s_edges + q * ne;
        unsigned *cnt = s_cnt + q * nb;
        const double lo = ed[0], hi = ed[nb], scale = (double)nb / (hi - lo);      // (this lane's parameter: registers)
        int cur = -1;
        unsigned run = 0;
        for_each_value(a, p, t, lanes, [&](double x) {
            const int b = find_bin(ed, nb, lo, hi, scale, x);
            if (b == cur) { ++run; return; }
            if (cur >= 0) atomicAdd(&cnt[cur], run);
            cur = b; run = 1;
        });
        if (cur >= 0) atomicAdd(&cnt[cur], run);
    }
    __syncthreads();
    unsigned long long *out = a.counts + p.e * a.ndim * nb;
    for (int i = t; i < a.ndim * nb; i += 256) {
        const unsigned c = s_cnt[i];
        if (c) atomicAdd(&out[i], (unsigned long long)c);
    }
}

template <int ND>
__global__ __launch_bounds__(256) void k_pair_histograms(const HistArgs a)
{
    extern __shared__ double s_hist[];
    const int nb = a.bins, ne = nb + 1, cells = nb * nb;
    double *s_edges = s_hist;                                  // (ND, bins + 1)
    double *s_scale = s_edges + ND * ne;                       // (ND,)
    unsigned *s_cnt = (unsigned *)(s_scale + ND);              // (pairs of this group, bins, bins)
    const int t = threadIdx.x;
    const ChainPart p = chain_part(a);
    const int q0 = (int)blockIdx.y * a.group, q1 = q0 + a.group < a.npairs ? q0 + a.group : a.npairs;
    const double *ge = a.edges + p.e * ND * ne;
    for (int i = t; i < ND * ne; i += 256) s_edges[i] = ge[i];
    for (int i = t; i < (q1 - q0) * cells; i += 256) s_cnt[i] = 0u;
    if (t < ND) s_scale[t] = (double)nb / (ge[t * ne + nb] - ge[t * ne]);
    __syncthreads();
    const unsigned wt = (unsigned)(p.w1 - p.w0), total = (unsigned)(p.s1 - p.s0) * wt;      // < 2^31 (chain_splits)
    const double *base = a.chain + (p.e * a.Wp + p.w0) * ND;
    for (unsigned r = t; r < total; r += 256) {
        const unsigned ds = r / wt, w = r - ds * wt;
        const double *__restrict__ row = base + (p.s0 + ds) * a.sample_stride + (long long)w * ND;
        double x[ND];
#pragma unroll
        for (int q = 0; q < ND; ++q) x[q] = __builtin_nontemporal_load(row + q);
        int b[ND];
#pragma unroll
        for (int q = 0; q < ND; ++q) {
            const double *ed = s_edges + q * ne;
            b[q] = find_bin(ed, nb, ed[0], ed[nb], s_scale[q], x[q]);
        }
        int pair = 0;
#pragma unroll
        for (int j = 0; j < ND; ++j) {
#pragma unroll
            for (int k = j + 1; k < ND; ++k, ++pair) {
                if (pair < q0 || pair >= q1) continue;          // (uniform: the group of this workgroup)
                if (b[j] < 0 || b[k] < 0) continue;
                const int cell = (pair - q0) * cells + b[j] * nb + b[k];
                // many lanes in the cell of the first one (a narrow posterior): one lane adds their number, the
                // others add on their own -- 64 adds to one LDS word take 64 turns
                const int first = __builtin_amdgcn_readfirstlane(cell);
                const unsigned long long same = __ballot(cell == first);
                if (__popcll(same) >= 8 && cell == first) {
                    if ((t & 63) == __ffsll((long long)same) - 1) atomicAdd(&s_cnt[first], (unsigned)__popcll(same));
                } else {
                    atomicAdd(&s_cnt[cell], 1u);
                }
            }
        }
    }
    __syncthreads();
    unsigned long long *out = a.counts + (p.e * a.npairs + q0) * cells;
    for (int i = t; i < (q1 - q0) * cells; i += 256) {
        const unsigned c = s_cnt[i];
        if (c) atomicAdd(&out[i], (unsigned long long)c);
    }
}

template <int ND>
struct PairHistLaunch {
    static void run(dim3 grid, hipStream_t st, const HistArgs &a)
    {
        const size_t lds = (size_t)ND * (a.bins + 2) * 8 + (size_t)a.group * a.bins * a.bins * 4;
        hipLaunchKernelGGL(k_pair_histograms<ND>, grid, dim3(256), lds, st, a);
    }
};

// no count is capped: chain_splits keeps the parts of an ensemble within one grid, hist_grid holds the ensembles to it
int check_hist_chain(int64_t n_samples, int64_t sample_stride, int64_t n_ensembles, int64_t walkers_per_ensemble, int ndim)
{
    return check_chain({n_samples, sample_stride, n_ensembles, walkers_per_ensemble, ndim}, 1, NO_CAP, NO_CAP, NO_CAP);
}

int hist_grid(HistArgs &a, long long wanted, unsigned *gx)
{
    const ChainSplit sp = chain_splits(a.n_samples, a.E, a.Wp, wanted);
    a.ss = sp.ss; a.sw = sp.sw;
    BISIP_TRY(check_grid(a.E, sp.ss * sp.sw, LOUD, "%lld ensembles in %lld x %lld parts", a.E, sp.ss, sp.sw));
    *gx = (unsigned)(a.E * sp.ss * sp.sw);
    return BISIP_OK;
}

}  // namespace

extern "C" {

int bisip_chain_range_dev(const double *d_chain, int64_t n_samples, int64_t sample_stride, int64_t n_ensembles,
                          int64_t walkers_per_ensemble, int ndim, double *d_out, int64_t *d_nonfinite, void *stream)
{
    if (!d_chain || !d_out || !d_nonfinite) return fail(BISIP_EINVAL, "null argument");
    BISIP_TRY(check_hist_chain(n_samples, sample_stride, n_ensembles, walkers_per_ensemble, ndim));
    HistArgs a{};
    a.chain = d_chain; a.n_samples = n_samples; a.sample_stride = sample_stride;
    a.E = n_ensembles; a.Wp = walkers_per_ensemble; a.ndim = ndim;
    a.keys = (unsigned long long *)d_out; a.nonfinite = (unsigned long long *)d_nonfinite;
    unsigned gx = 0;
    BISIP_TRY(hist_grid(a, 4096, &gx));
    hipStream_t st = (hipStream_t)stream;
    const dim3 cols((unsigned)((n_ensembles * ndim + 255) / 256));
    hipLaunchKernelGGL(k_chain_range_init, cols, dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_chain_range, dim3(gx), dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_chain_range_finish, cols, dim3(256), 0, st, a);
    HIP_TRY(hipGetLastError());
    return BISIP_OK;
}

int bisip_chain_histograms_dev(const double *d_chain, int64_t n_samples, int64_t sample_stride, int64_t n_ensembles,
                               int64_t walkers_per_ensemble, int ndim, const double *d_edges, int bins,
                               int64_t *d_counts, void *stream)
{
    if (!d_chain || !d_edges || !d_counts) return fail(BISIP_EINVAL, "null argument");
    BISIP_TRY(check_hist_chain(n_samples, sample_stride, n_ensembles, walkers_per_ensemble, ndim));
    if (bins < 1) return fail(BISIP_EINVAL, "bins=%d", bins);
    const size_t lds = (size_t)ndim * ((size_t)(bins + 1) * 8 + (size_t)bins * 4);
    if (lds > HIST_LDS_BYTES)
        return fail(BISIP_EUNSUPPORTED, "bins=%d: the edges and counters of %d parameters take %zu bytes of LDS, more than %zu",
                    bins, ndim, lds, HIST_LDS_BYTES);
    HistArgs a{};
    a.chain = d_chain; a.n_samples = n_samples; a.sample_stride = sample_stride;
    a.E = n_ensembles; a.Wp = walkers_per_ensemble; a.ndim = ndim; a.bins = bins;
    a.edges = d_edges; a.counts = (unsigned long long *)d_counts;
    unsigned gx = 0;
    BISIP_TRY(hist_grid(a, 4096, &gx));
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(d_counts, 0, (size_t)n_ensembles * ndim * bins * 8, st));
    hipLaunchKernelGGL(k_chain_histograms, dim3(gx), dim3(256), lds, st, a);
    HIP_TRY(hipGetLastError());
    return BISIP_OK;
}

int bisip_chain_pair_histograms_dev(const double *d_chain, int64_t n_samples, int64_t sample_stride,
                                    int64_t n_ensembles, int64_t walkers_per_ensemble, int ndim, const double *d_edges,
                                    int bins, int64_t *d_counts, void *stream)
{
    if (!d_chain || !d_edges || !d_counts) return fail(BISIP_EINVAL, "null argument");
    BISIP_TRY(check_hist_chain(n_samples, sample_stride, n_ensembles, walkers_per_ensemble, ndim));
    if (ndim < 2) return fail(BISIP_EINVAL, "ndim=%d has no pairs", ndim);
    if (bins < 1) return fail(BISIP_EINVAL, "bins=%d", bins);
    const size_t fixed = (size_t)ndim * (bins + 2) * 8, cell_bytes = (size_t)bins * bins * 4;
    if (bins > 1024 || fixed + cell_bytes > HIST_LDS_BYTES)
        return fail(BISIP_EUNSUPPORTED, "bins=%d: the %d x %d counters of one pair do not fit %zu bytes of LDS", bins, bins,
                    bins, HIST_LDS_BYTES);
    HistArgs a{};
    a.chain = d_chain; a.n_samples = n_samples; a.sample_stride = sample_stride;
    a.E = n_ensembles; a.Wp = walkers_per_ensemble; a.ndim = ndim; a.bins = bins;
    a.npairs = ndim * (ndim - 1) / 2;
    const size_t fit = (HIST_LDS_BYTES - fixed) / cell_bytes;
    a.group = (int)(fit < (size_t)a.npairs ? fit : (size_t)a.npairs);
    const int groups = (a.npairs + a.group - 1) / a.group;
    a.edges = d_edges; a.counts = (unsigned long long *)d_counts;
    unsigned gx = 0;
    // every workgroup ends with one global add per cell it touched: fewer, longer workgroups than the 1-D sweep
    BISIP_TRY(hist_grid(a, 1024, &gx));
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(d_counts, 0, (size_t)n_ensembles * a.npairs * cell_bytes * 2, st));
    return launch_by_ndim<PairHistLaunch>(ndim, dim3(gx, (unsigned)groups), st, a);
}

}  // extern "C"
