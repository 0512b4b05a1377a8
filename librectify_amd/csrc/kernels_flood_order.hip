// The flood's schedule hook (lr_set_flood_schedule): a round's active list put into a chosen order in front of the round's
// exploration.  A translation unit and so a code object of their own: the kernels of kernels_flood.hip are what they were
// without the hook, and a process that never sets it launches nothing from here.
//
// The list that the control block's round counter selects (kernels_flood.hip: act_now) is gathered into the OTHER list in
// the new order and copied back.  The other list is free at that point: the round that read it is over, and the next to
// write it is this round's survivors pass, which runs behind every reader of the current list.  Both launches read the words
// the round's own kernels read -- list length, round counter, request for a giant step -- and leave at once behind a
// pending giant step (the round behind it does nothing and does not count: its list must stay as it is for the round that
// does) or when nothing is left.
#include <algorithm>

#include "common.h"

namespace lramd {
namespace {

constexpr int kOrderThreads = 256;

// order 1: reversed; order 2: flood_schedule_perm of (seed, round counter, list length)
__global__ __launch_bounds__(kOrderThreads) void flood_order_gather_kernel(const uint32_t* __restrict__ ctrl, uint32_t* act_a, uint32_t* act_b,
                                                                          uint32_t cap, int order, uint32_t seed) {
    if (ctrl[kFloodCtrlGiantStep] != 0u) return;
    const uint32_t n = ctrl[kFloodCtrlNAct], rounds = ctrl[kFloodCtrlRounds];
    if (n == 0u || n > cap) return;
    const uint32_t* __restrict__ src = (rounds & 1u) ? act_b : act_a;
    uint32_t* __restrict__ dst = (rounds & 1u) ? act_a : act_b;
    uint32_t a = 1u, b = 0u;
    if (order == 2) flood_schedule_coeffs(seed, rounds, n, &a, &b);
    for (uint32_t i = blockIdx.x * kOrderThreads + threadIdx.x; i < n; i += gridDim.x * kOrderThreads) {
        const uint32_t j = order == 2 ? flood_schedule_perm(i, a, b, n) : n - 1u - i;  // (j < n either way)
        dst[i] = src[j];
    }
}

__global__ __launch_bounds__(kOrderThreads) void flood_order_copy_kernel(const uint32_t* __restrict__ ctrl, uint32_t* act_a, uint32_t* act_b,
                                                                        uint32_t cap) {
    if (ctrl[kFloodCtrlGiantStep] != 0u) return;
    const uint32_t n = ctrl[kFloodCtrlNAct], rounds = ctrl[kFloodCtrlRounds];
    if (n == 0u || n > cap) return;
    uint32_t* __restrict__ now = (rounds & 1u) ? act_b : act_a;
    const uint32_t* __restrict__ other = (rounds & 1u) ? act_a : act_b;
    for (uint32_t i = blockIdx.x * kOrderThreads + threadIdx.x; i < n; i += gridDim.x * kOrderThreads) now[i] = other[i];
}

}  // namespace

void launch_flood_order(const FloodBuffers& B, uint32_t cap, hipStream_t s) {
    if (B.sched_order != 1 && B.sched_order != 2) return;
    if (cap == 0u || !B.ctrl || !B.act_a || !B.act_b) return;
    const uint32_t blocks = std::min<uint32_t>((cap + kOrderThreads - 1) / kOrderThreads, 1024u);
    hipLaunchKernelGGL(flood_order_gather_kernel, dim3(blocks), dim3(kOrderThreads), 0, s, B.ctrl, B.act_a, B.act_b, cap, B.sched_order,
                       B.sched_seed);
    hipLaunchKernelGGL(flood_order_copy_kernel, dim3(blocks), dim3(kOrderThreads), 0, s, B.ctrl, B.act_a, B.act_b, cap);
}

}  // namespace lramd
