// Hand-over between the waves of one workgroup without workgroup barriers: monotone counters in LDS, and the LDS-DMA that fills
// the slots they guard.  A wave's DS instructions execute in order, so a counter bump issued after the data accesses is ordered
// behind them without any s_waitcnt - in particular a wave never waits for its global stores here, which a workgroup-scope release
// fence (vmcnt(0)) would make it do every tile.  What each counter counts is the business of the kernel that owns it.
#pragma once
#include "common.h"

namespace gnnome {

__device__ __forceinline__ unsigned lds_addr(const void* p) { return (unsigned)(size_t)(__attribute__((address_space(3))) const void*)p; }

// Spin until the counter at `addr` has reached `want`.  nap 0..3 = s_sleep 1 / 4 / 16 / 64 between polls: a consumer whose wait is on
// the critical path polls tightly (0); a producer that runs a whole slot ahead may poll rarely, its ds_reads compete with the compute
// waves' operand reads.  A literal nap folds to a single s_sleep.
__device__ __forceinline__ void flag_wait(unsigned addr, unsigned want, int nap) {
    unsigned v, spins = 0;
    for (;;) {
        asm volatile("ds_read_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(v) : "v"(addr) : "memory");
        if (__builtin_amdgcn_readfirstlane(v) >= want) break;
        if (++spins > (1u << 26)) __builtin_trap();   // a lost hand-over must end the launch, not hang the queue
        if (nap == 0) {
            __builtin_amdgcn_s_sleep(1);
        } else if (nap == 1) {
            __builtin_amdgcn_s_sleep(4);
        } else if (nap == 2) {
            __builtin_amdgcn_s_sleep(16);
        } else {
            __builtin_amdgcn_s_sleep(64);
        }
    }
}
__device__ __forceinline__ void flag_bump(unsigned addr, int lane) {
    if (lane == 0) asm volatile("ds_add_u32 %0, %1" ::"v"(addr), "v"(1u) : "memory");
}

// 1 KB of LDS-DMA (global_load_lds_dwordx4), in two forms that differ in what the compiler may move across them.  Both: lane l's 16
// bytes at src + voff (voff = 16 l) land at lds + 16 l.  They name m0, a reserved register: a file that calls them is compiled with
// -Wno-inline-asm.
//
// dma_row: ordered against every memory access around it.
__device__ __forceinline__ void dma_row(const float* row, unsigned voff, unsigned lds) {
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"(voff), "s"(row), "s"(lds) : "memory", "m0");
}
// dma_piece: NO "memory" clobber.  Between the two barriers that bracket it nothing reads the slot it fills, and with the clobber hipcc
// may not move the NEXT k steps' ds_reads above it - it then waits out one LDS latency per k step (measured in k_node_project: 224
// cycles per step against 96 of MFMA).  asm volatile keeps it ordered with the barriers and the waits.
__device__ __forceinline__ void dma_piece(const void* src, unsigned voff, unsigned lds) {
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"(voff), "s"(src), "s"(lds) : "m0");
}

}  // namespace gnnome
