// chain_lags.h -- the lag-sum tile of k_ac_lags (chain_autocorr.hip) and k_ess_lags (chain_ess.hip): its constants and the
// host arithmetic of a round.  acf_k = sum_{t < len - k} y_t y_{t + k} of a series' centred samples y is taken as direct
// sums, a round of lags at a time.  Workgroup (tile, b) of 4 waves owns 64 series (one per lane) and the lags kb = k0 + 64 b
// ... kb + 63 of the round that starts at lag k0, wave w the 16 lags kb + 16 w + i: acc_i = sum_t y_t y_{t + kb + 16 w + i}
// over t < len - kb in 16 registers of every lane, with y = 0 beyond the series (a zero product adds nothing).  Per pass the
// LDS holds y[t0, t0 + 32) (A) and y[t0 + kb, t0 + kb + 96) (B) of the tile, one lane's series per column.
// The loop stands in both kernels: as one force-inlined template over the loader it kept registers, LDS and instruction
// counts, but k_ac_lags ran 1 ... 3 % slower (profiles/lag_tile_shared_vs_copied.md).  Change the tile in both.
#pragma once
#include "chain.h"

namespace bisip {

constexpr int LAG_TILE = 64;        // series per tile (one per lane)
constexpr int LAGS_WAVE = 16;       // lag accumulators per lane
constexpr int LAG_WAVES = 4;        // waves of a lag workgroup
constexpr int LAG_BLOCK = LAGS_WAVE * LAG_WAVES;        // lags per lag workgroup
constexpr int LAG_T = 32;           // samples staged per pass
constexpr int LAG_TARGET_BLOCKS = 512;                  // two lag workgroups per compute unit (64 KiB of LDS each)
constexpr int LAG_PREP_WAVES = 16;  // waves of a prep workgroup: wave q takes samples q, q + 16, ... of the tile
constexpr int LAG_GROUP = 256;      // series one workgroup of a unit's group sums adds, in order

// lags per round: enough lag workgroups to fill the chip next to the tiles_total tiles (of every series set), no more
// than a series of len samples has, and within grid dimension y
inline long long round_lags(long long len, long long tiles_total)
{
    long long nb = (LAG_TARGET_BLOCKS + tiles_total - 1) / tiles_total;
    const long long need = (len + LAG_BLOCK - 1) / LAG_BLOCK;
    if (nb > need) nb = need;
    if (nb > 65535) nb = 65535;
    if (nb < 1) nb = 1;
    return nb * LAG_BLOCK;
}

// lag blocks of the round of Lr lags that starts at lag k0: the last round ends with the series
inline long long round_blocks(long long len, long long k0, long long Lr)
{
    return (len - k0 < Lr ? len - k0 + LAG_BLOCK - 1 : Lr) / LAG_BLOCK;
}

}  // namespace bisip
