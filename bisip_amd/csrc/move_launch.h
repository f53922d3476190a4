// move_launch.h -- what the two move dispatch units share (dispatch_moves.hip: single spectrum and the entry
// points; dispatch_moves_batch.hip: batch of spectra).
#pragma once
#include "move_kernels.h"
#include "stretch_launch.h"

namespace bisip {
namespace host {

// lanes per slot of a move's half-step: the stretch launch's rule for the same number of slots
inline int move_lanes(const MoveArgs &a) { return stretch_lanes(StretchWork{STRETCH_HALF, &a.s, nullptr}); }

// one half-step launch; workgroups as launch_stretch shapes them (four_wave_workgroups)
template <class LP>
int launch_move(const MoveArgs &a, int kind, const LP &lp, hipStream_t st)
{
    auto go = [&](auto move) {
        constexpr int MOVE = decltype(move)::value;
        const long long lanes = a.s.n_slots * LP::L;
        if (four_wave_workgroups(lanes))
            hipLaunchKernelGGL((k_move_half<LP, MOVE, 256>), dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, st, a, lp);
        else
            hipLaunchKernelGGL((k_move_half<LP, MOVE, 64>), dim3((unsigned)((lanes + 63) / 64)), dim3(64), 0, st, a, lp);
    };
    if (kind == MOVE_DE) go(std::integral_constant<int, MOVE_DE>{});
    else go(std::integral_constant<int, MOVE_SNOOKER>{});
    HIP_TRY(hipGetLastError());
    return BISIP_OK;
}

int dispatch_move(const bisip_ctx *c, const MoveArgs &a, int kind, long long Wp, hipStream_t st);
int dispatch_move_batch(const bisip_ctx *c, const MoveArgs &a, int kind, long long Wp, hipStream_t st);   // dispatch_moves_batch.hip

}  // namespace host
}  // namespace bisip
