// trace_flat.hip -- the flat (single-level) traversal launches: k_trace_s of
// flattened scenes and its exact-tie retrace k_tie.  They live in their own
// translation unit so that they alone are compiled with the memory-clause
// scheduler (Makefile DEV_FLAT_FLAGS: -amdgpu-sched-strategy=max-memory-clause,
// which groups each iteration's node-pair and TriAccel loads into one clause:
// C3 trace -1.0%, C5 -0.6%; the two-level kernel, left in mtsg.hip, loses 3%
// under it -- DESIGN.md §3, profiles/r06_sched_strategy.txt).  Scheduling
// only: the same IEEE operations, the same hits.
// (kernels.h defines every kernel; this unit launches only the flat traversal)
#pragma clang diagnostic ignored "-Wunused-function"
// The flat kernels' short stack keeps the lane's index in a register, filled
// once per kernel, instead of recomputing it with a v_mbcnt pair at every push
// and pop (kernels.h SpecStack): 64 VGPRs from 61, still 8 waves/SIMD and no
// scratch; C3 trace -2.3 ms of 100.7, with the pre-records on -2.1 of 97.0
// (profiles/ray_presetup_ab.txt).  This unit only: the tail kernel and the
// two-level traversal keep the recomputed index.
#ifndef MTSG_STACK_LANE   // (-DMTSG_STACK_LANE=0: the recomputed index everywhere, for A/B runs)
#define MTSG_STACK_LANE 1
#endif
#include "kernels.h"

#if MTSG_FLAT_REGS
namespace {
// measurement variant: the flat production kernels with their own register
// budget (kernels.h FLAT_TRACE_ATTR, measured: off); the COUNT instantiations
// keep the template's attributes
#define FLAT_TRACE_KERNEL(MIN_IDLE, KNOBS)                                                                               \
    template <>                                                                                                          \
    __global__ void FLAT_TRACE_ATTR k_trace_s<false, MIN_IDLE, false, KNOBS>(DevScene S, DevPaths P, int cIn, int sIn,   \
                                                                             uint32_t nIdentity, unsigned long long *wt) { \
        trace_s_body<false, MIN_IDLE, false, KNOBS>(S, P, cIn, sIn, nIdentity, wt);                                      \
    }
FLAT_TRACE_KERNEL(16, false)
FLAT_TRACE_KERNEL(32, false)
FLAT_TRACE_KERNEL(16, true)
#undef FLAT_TRACE_KERNEL
}  // namespace
#endif

namespace mtsg {

template <bool COUNT>
static void launch_flat(const FlatTraceLaunch &a) {
    const dim3 blk(TRACE_BLOCK);
    // k_trace_s<.., false, false>: rectangles tested at ray setup (kernels.h
    // spec_init<true>); <.., false, true>, the test knobs' kernel, and
    // k_trace_s_leaf, the kernel of the scenes that do not take the setup mode
    // (a.rectSetup false): in the leaves.  The COUNT pass follows the timed kernel.
    // a.pre: the rays carry pre-records, the refill runs no rectangle loop
    // (k_trace_s_pre; the launcher sets it only with a.rectSetup and without a.knobs)
    // a.leafFilter: those setup-mode kernels, timed (not COUNT: every counter
    // describes the walk over Mitsuba's leaves), read the leaf words of
    // blocksRS, which hold no rectangle records; k_tie below keeps a.S
    if (!COUNT && a.leafFilter && a.blocksRS && a.rectSetup && !a.knobs) {
        DevScene S = *a.S;
        S.blocks = a.blocksRS;
        S.root2 = a.root2RS;
        if (a.pre && a.refill32) hipLaunchKernelGGL((k_trace_s_pre<COUNT, 32>), a.grid, blk, 0, a.stream, S, *a.P, a.cIn, a.sIn, a.n, a.wt);
        else if (a.pre) hipLaunchKernelGGL((k_trace_s_pre<COUNT, 16>), a.grid, blk, 0, a.stream, S, *a.P, a.cIn, a.sIn, a.n, a.wt);
        else if (a.refill32) hipLaunchKernelGGL((k_trace_s<COUNT, 32>), a.grid, blk, 0, a.stream, S, *a.P, a.cIn, a.sIn, a.n, a.wt);
        else hipLaunchKernelGGL((k_trace_s<COUNT, 16>), a.grid, blk, 0, a.stream, S, *a.P, a.cIn, a.sIn, a.n, a.wt);
    } else if (a.pre && a.rectSetup && !a.knobs) {
        if (a.refill32) hipLaunchKernelGGL((k_trace_s_pre<COUNT, 32>), a.grid, blk, 0, a.stream, *a.S, *a.P, a.cIn, a.sIn, a.n, a.wt);
        else hipLaunchKernelGGL((k_trace_s_pre<COUNT, 16>), a.grid, blk, 0, a.stream, *a.S, *a.P, a.cIn, a.sIn, a.n, a.wt);
    } else if (a.knobs && !COUNT) hipLaunchKernelGGL((k_trace_s<false, 16, false, true>), a.grid, blk, 0, a.stream, *a.S, *a.P, a.cIn, a.sIn, a.n, a.wt);
    else if (!a.rectSetup && a.refill32) hipLaunchKernelGGL((k_trace_s_leaf<COUNT, 32>), a.grid, blk, 0, a.stream, *a.S, *a.P, a.cIn, a.sIn, a.n, a.wt);
    else if (!a.rectSetup) hipLaunchKernelGGL((k_trace_s_leaf<COUNT, 16>), a.grid, blk, 0, a.stream, *a.S, *a.P, a.cIn, a.sIn, a.n, a.wt);
    else if (a.refill32) hipLaunchKernelGGL((k_trace_s<COUNT, 32>), a.grid, blk, 0, a.stream, *a.S, *a.P, a.cIn, a.sIn, a.n, a.wt);
    else hipLaunchKernelGGL((k_trace_s<COUNT, 16>), a.grid, blk, 0, a.stream, *a.S, *a.P, a.cIn, a.sIn, a.n, a.wt);
    if (a.tie) {
        if (a.knobs) hipLaunchKernelGGL((k_tie<true>), a.tieGrid, blk, 0, a.stream, *a.S, *a.P);
        else hipLaunchKernelGGL((k_tie<false>), a.tieGrid, blk, 0, a.stream, *a.S, *a.P);
    }
}

void launch_trace_flat(const FlatTraceLaunch &a) {
    if (a.count) launch_flat<true>(a);
    else launch_flat<false>(a);
}

int trace_flat_blocks_per_cu() {
    int perCU = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&perCU, (const void *)k_trace_s<false, 16>, TRACE_BLOCK, 0) != hipSuccess) return 0;
    return perCU;
}

}  // namespace mtsg
