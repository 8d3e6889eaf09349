// Device-side vocabulary of the fp16 detector kernels: what more than one of rva_conv.hip (the convolution families), rva_stem.hip
// (the stems) and rva_yolo_ops.hip (SPPF / pooling / upsample / detect head) needs; what only one uses stays there.  Everything is
// internal to the including file (unnamed namespace, __forceinline__): a kernel's machine code does not depend on its file.
#pragma once

#include <hip/hip_fp16.h>

#include <cstdlib>

#include "rva_internal.h"

namespace {

typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef float f4 __attribute__((ext_vector_type(4)));
// NOTE: staging registers use this native vector, not HIP's uint4 struct: assigning a dereferenced
// `const uint4*` into an array element lowers to a memcpy that SROA does not split, the array then lives in
// scratch and every prefetch load is followed by vmcnt(0) + scratch_store (serialised loads).
typedef unsigned int u4 __attribute__((ext_vector_type(4)));

// Timing-only ablation switches (skip the MFMA phase / the prefetch loads / the epilogue) exist in the private diagnostic
// build only (tools/row_stamps.py compiles with -DRVA_ROW_STAMPS); the shipped library has neither the fields nor the reads.
#ifdef RVA_ROW_STAMPS
#define RVA_DBG_FIELD int dbg;
#define RVA_DBG(a, bit) ((a).dbg & (bit))
#else
#define RVA_DBG_FIELD
#define RVA_DBG(a, bit) 0
#endif
#ifdef RVA_ROW_STAMPS
// tuning aid (tools/row_stamps.py builds a private library with this macro): per-phase s_memtime stamps of a few blocks.
// Without relocatable device code no device variable is shared between files: each file that stamps has its own g_stamps and
// exports its own reader (RVA_STAMP_READER: rva_dbg_read_stamps in rva_conv.hip, rva_dbg_read_stem_stamps in rva_stem.hip).
__device__ unsigned long long g_stamps[8][256];
__device__ __forceinline__ unsigned long long stamp_now()
{
    unsigned long long t;
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
    return t;
}
#define STAMP(k) do { if (st_on && st_n < 256) g_stamps[st_slot][st_n++] = stamp_now(); } while (0)
// what STAMP reads: threads WHO of the first NB of the blocks that lie gridDim.x / DIV apart stamp into slot SLOT
#define STAMP_BEGIN_ON(WHO, DIV, NB, SLOT)                                                                                 \
    const int st_stride = gridDim.x / (DIV);                                                                               \
    const bool st_on = (WHO) && st_stride > 0 && blockIdx.x % st_stride == 0 && blockIdx.x / st_stride < (NB);             \
    const int st_slot = st_on ? (SLOT) : 0;                                                                                \
    int st_n = 0
#define RVA_STAMP_READER(name) \
    extern "C" int name(unsigned long long *host) { return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(g_stamps), sizeof(unsigned long long) * 8 * 256); }
#else
#define STAMP(k) do { } while (0)
#define STAMP_BEGIN_ON(WHO, DIV, NB, SLOT) do { } while (0)
#endif
#define STAMP_BEGIN() STAMP_BEGIN_ON(tid == 0, 8, 8, blockIdx.x / st_stride)     // thread 0 of eight blocks spread over the grid

// Swizzled layout for 32-channel (64-byte) rows, no padding: the 16-byte chunk c of row r lives at physical chunk
// (c + 2*(r>>2)) & 3.  ds_read_b128 serves a wave in groups of 16 lanes that mix rows {0-3,12-15} at chunk c with
// rows {4-11} at chunk c+1 (MI355X_MICROARCH.md, LDS table); with 80-byte padded rows 3 of the 16 lanes of every
// group collide (PMC: SQ_LDS_BANK_CONFLICT = 50 % of SQ_LDS_IDX_ACTIVE on the 3x3 kernels).  For this mapping the four
// rows of a group that share (r & 3) get physical chunks {2q, 2q+2, 2q+3, 2q+1} mod 4 -- distinct for any row base --
// and the staging ds_write_b128 (4 lanes per row, consecutive rows) alternates 16-bank halves: both conflict-free.
__device__ __forceinline__ int swz32(int row, int chunk) { return row * 32 + (((chunk + 2 * (row >> 2)) & 3) << 3); }

// x * sigmoid(x) with v_exp_f32 + v_rcp_f32 (1 ulp): __fdividef / operator/ expand to the ~12-instruction IEEE
// division sequence here, which dominated the epilogues (64-128 SiLUs per thread per tile)
__device__ __forceinline__ float silu_f(float v) { return v * __builtin_amdgcn_rcpf(1.0f + __expf(-v)); }

// LDS-DMA (global_load_lds): address-space pointers of the builtin's operands, and the counted wait for the loads in flight
typedef __attribute__((address_space(3))) void *lds_vptr;
typedef const __attribute__((address_space(1))) void *glb_vptr;

template <int N> __device__ __forceinline__ void wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }

// Detect head (head_anchor in rva_yolo_ops.hip, the decoding epilogue of k_conv_gbig<..., HEAD> in rva_conv.hip): sigmoid of
// eight class logits of one anchor into eight consecutive class rows (row stride A halves) starting at `o`.  GUARD: only the
// first `left` of the eight rows exist (the last group of a class count that is no multiple of 8; the other logits are padding).
template <bool GUARD>
__device__ __forceinline__ void store_scores8(__half *o, size_t A, const uint4 q, int left)
{
    const __half2 *hq = reinterpret_cast<const __half2 *>(&q);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const float2 f = __half22float2(hq[t]);
        if (!GUARD || 2 * t < left) o[(size_t)(2 * t) * A] = __float2half_rn(__builtin_amdgcn_rcpf(1.0f + __expf(-f.x)));
        if (!GUARD || 2 * t + 1 < left) o[(size_t)(2 * t + 1) * A] = __float2half_rn(__builtin_amdgcn_rcpf(1.0f + __expf(-f.y)));
    }
}

}  // namespace
