// Shared pieces of the ring-staged apply kernels (apply_ring.hip: structured meshes with geometry classes; apply_ring_u.hip: any
// 3D mesh, geometry from staged vertex coordinates): the LDS-DMA primitives, the LDS-only workgroup barrier, the block walk of a
// persistent workgroup and the swizzled 32-byte-row image of a nodal vector.
#pragma once
#include "cell_geom.hpp"
#include <algorithm>

namespace ring {

constexpr int RB = 256;           // cells per block (= KNP_HALO_BLK: the halo tables are built for it)
static_assert(RB == KNP_HALO_BLK, "the halo tables are built for 256-cell blocks");

// one LDS-DMA instruction: lane l copies 16 bytes from its own source address to (lds_dst + 16 l); lds_dst is wave-uniform.  M0 is
// written in the statement that reads it and declared clobbered, so the compiler never assumes a value of its own survives.
__device__ __forceinline__ void glds16(const void* gsrc, unsigned lds_dst) {
    asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" : : "v"(gsrc), "s"(lds_dst) : "memory", "m0");
}
// four consecutive 1 KiB pieces from ONE address register and ONE M0 value: the instruction offset moves both the global and the
// LDS address (checked by tools/microbench/glds_ring.hip)
__device__ __forceinline__ void glds16_run4(const void* gsrc, unsigned lds_dst) {
    asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off\n\tglobal_load_lds_dwordx4 %0, off offset:1024\n\t"
                 "global_load_lds_dwordx4 %0, off offset:2048\n\tglobal_load_lds_dwordx4 %0, off offset:3072"
                 : : "v"(gsrc), "s"(lds_dst) : "memory", "m0");
}
template <int N> __device__ __forceinline__ void wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" : : "n"(N) : "memory"); }
// workgroup barrier that orders LDS traffic only: the loader's DMAs stay in flight across it (it counts them itself), the
// consumers' stores are never waited for
__device__ __forceinline__ void ring_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

// Blocks of one workgroup: the block range is cut into 8 contiguous chunks, one per XCD (XCD = blockIdx.x & 7 under round-robin
// dispatch: an XCD's workgroups walk adjacent blocks, so the halo rows come out of its own L2; speed only); inside a chunk the
// XCD's workgroups take the blocks round-robin.
struct RingWalk {
    int64_t b_lo, first, last, member, members;
    __device__ __forceinline__ explicit RingWalk(const MeshDev& m) {
        b_lo = m.c_begin / RB;
        const int64_t nblk = (m.c_end - 1) / RB - b_lo + 1;
        const int64_t chunk = (nblk + 7) / 8;
        first = (int64_t)(blockIdx.x & 7u) * chunk;
        last = first + chunk < nblk ? first + chunk : nblk;
        member = blockIdx.x >> 3;
        members = gridDim.x >> 3;
    }
    // absolute block (cells [256 b, 256 b + 256)) of iteration n, or -1
    __device__ __forceinline__ int64_t blk(int64_t n) const {
        const int64_t b = first + member + n * members;
        return b < last ? b_lo + b : -1;
    }
};

// ---- loader schedules ------------------------------------------------------------------------------------------------------------
// What the four loader waves of a workgroup run from start to end.  list_dma(n) issues the list piece(s) of the workgroup's n-th
// block (a no-op past its last block and on every loader but the one that owns the lists), data_dma(n) issues this loader's share
// of block n's records; every ring_barrier() below is met by one of the consumers, so the CONSUMERS' BARRIER COUNT is part of the
// schedule -- a mismatch is a hang:
//     A (lists 0 and 1 visible to every loader; the kernel's tables staged),  B (block 0 landed),  then one per interval.
// Interval n is the one in which the consumers work on block n: nblk intervals for a workgroup with nblk blocks, nblk + 1 with a
// closing interval.

// One block ahead, every interval ends in a full drain (unstructured family: two slots, two list buffers).
// Consumers: A, B, one barrier after each block = 2 + nblk.
template <typename ListDma, typename DataDma>
__device__ __forceinline__ void load_one_ahead_drained(const RingWalk& w, ListDma list_dma, DataDma data_dma) {
    list_dma(0); list_dma(1);
    wait_vm<0>();
    ring_barrier();                                                    // A
    data_dma(0);
    wait_vm<0>();
    ring_barrier();                                                    // B
    for (int64_t n = 0; w.blk(n) >= 0; ++n) {
        list_dma(n + 2);                                               // into the buffer block n's gathers read in the last interval
        if (w.blk(n + 1) >= 0) data_dma(n + 1);
        wait_vm<0>();
        ring_barrier();
    }
}

// Two blocks ahead (structured family: three or four slots, four list buffers).  N0..N3 = the DMA instructions of loaders 0..3 in
// one data_dma: the counted wait of loader lw retires everything but its share of the youngest block (the list piece issued before
// that share included) -- exactly the block the consumers need next -- and leaves the youngest in flight across the barrier.
// Consumers: A, B, one barrier after each block = 2 + nblk; with CLOSING (the staggered EMI consumers, whose last interval holds
// the second halves of the last block) one more = 3 + nblk.
template <bool CLOSING, int N0, int N1, int N2, int N3, typename ListDma, typename DataDma>
__device__ __forceinline__ void load_two_ahead_counted(const RingWalk& w, int lw, ListDma list_dma, DataDma data_dma) {
    auto wait_older = [&]() {
        if (lw == 0) wait_vm<N0>(); else if (lw == 1) wait_vm<N1>(); else if (lw == 2) wait_vm<N2>(); else wait_vm<N3>();
    };
    list_dma(0); list_dma(1);
    wait_vm<0>();
    ring_barrier();                                                    // A
    data_dma(0);
    list_dma(2);
    if (w.blk(1) >= 0) { data_dma(1); wait_older(); } else wait_vm<0>();
    ring_barrier();                                                    // B: block 0 and list 2 have landed
    for (int64_t n = 0; w.blk(n) >= 0; ++n) {
        list_dma(n + 3);
        if (w.blk(n + 2) >= 0) { data_dma(n + 2); wait_older(); }      // block n + 2 stays in flight; list n + 3, block n + 1 have landed
        else wait_vm<0>();
        ring_barrier();
    }
    if (CLOSING) { wait_vm<0>(); ring_barrier(); }
}

// LDS image of a nodal vector: 32-byte rows, read by the consumers with 16-byte ds_read_b128 -- lanes that read consecutive rows
// hit 16-byte bank groups (2 R + half) mod 16, i.e. rows 8 apart collide.  The two halves of every second group of 8 rows are
// therefore stored SWAPPED (the DMA writes lane-linear, so the swap is made on the per-lane source address): conflict-free.
__device__ __forceinline__ int swz_half(int lane) { return ((lane & 1) ^ ((lane >> 4) & 1)) * 2; }       // source half (in doubles) of lane 2 i + h
// 256 own rows of one nodal vector: 8 instructions, lanes 2 i / 2 i + 1 carry the two halves of a row; two runs of four pieces when
// the whole block lies inside the vector (every block but possibly the last one)
__device__ __forceinline__ void dma_own_rows(const double* __restrict__ v, int64_t c0, int64_t nc, unsigned dst, int lane) {
    if (c0 + RB <= nc) {
        const double* src = v + (c0 + (lane >> 1)) * 4 + swz_half(lane);
        glds16_run4(src, dst);
        glds16_run4(src + 128 * 4, dst + 4096);
        return;
    }
#pragma unroll
    for (int p = 0; p < 8; ++p) {
        int64_t row = c0 + p * 32 + (lane >> 1);
        row = row < nc ? row : 0;
        glds16(v + row * 4 + swz_half(lane), dst + p * 1024);
    }
}
// consumer side: the four values of row R of such an image
__device__ __forceinline__ void lds_row(const lds_double* base, unsigned R, double* r) {
    typedef double __attribute__((ext_vector_type(2))) vdouble2;
    typedef __attribute__((address_space(3))) vdouble2 lds_vdouble2;
    const unsigned s = (R >> 3) & 1u;
    const vdouble2 a = *(const lds_vdouble2*)(base + 4 * R + 2 * s);
    const vdouble2 b = *(const lds_vdouble2*)(base + 4 * R + 2 * (s ^ 1u));
    r[0] = a.x; r[1] = a.y; r[2] = b.x; r[3] = b.y;
}
__device__ __forceinline__ int64_t list_cell(const lds_int* L, int e, int hs) {
    const int src = e < hs ? L[e] : -1;
    return src >= 0 ? (int64_t)(src >> 2) : 0;
}

// ---- host side of the launches ----
constexpr size_t RING_MAX_LDS = 160 * 1024;   // LDS per workgroup: the CU's 160 KB
// more than 64 KB of dynamic LDS per workgroup has to be granted per kernel and device: once per context (knp_ctx::lds_granted)
template <typename KernelT> bool grant_lds(knp_ctx* c, KernelT kernel, size_t lds) {
    auto it = c->lds_granted.find((const void*)kernel);
    if (it != c->lds_granted.end() && it->second >= lds) return true;
    if (hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) return false;
    c->lds_granted[(const void*)kernel] = lds;
    return true;
}

// one workgroup per CU (the ring takes most of a CU's LDS), a multiple of 8, not more than 8 per 8 blocks
inline dim3 ring_grid(const knp_ctx* c, const MeshDev& m, int reserve_cus) {
    const int64_t nblk = (m.c_end - 1) / RB - m.c_begin / RB + 1;
    const int cus = std::max(c->ncu - std::max(reserve_cus, 0), 8);
    int64_t per_xcd = std::max<int64_t>(1, std::min<int64_t>(cus / 8, (nblk + 7) / 8));
    // tests only: KNP_RING_WG = workgroups of the launch (rounded down to a multiple of 8), so that small oracle-sized meshes put many
    // blocks on a workgroup (slot reuse, list-buffer wrap, counted vmcnt with two blocks in flight: the steady state of the r=2 runs)
    const int wg = env_int("KNP_RING_WG", 0);
    if (wg >= 8) per_xcd = std::min<int64_t>(per_xcd, wg / 8);
    return dim3((unsigned)(8 * per_xcd));
}

}  // namespace ring
