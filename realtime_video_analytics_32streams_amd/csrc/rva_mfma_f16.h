// The fp16-input counterpart of f32_chunk / f32_conv_taps (rva_mfma_f32.h) on v_mfma_f32_32x32x16_f16, included by
// rva_clip3d.hip (device code only).  A wave owns MT x NT tiles of 32 GEMM rows (output positions) x 32 columns (output
// channels); lane & 31 = row of an A tile and column of a B tile, lane >> 5 = lane half h.  Operands are fp16, every sum is fp32.
//
// THE reduction order of an output element, for every kernel built on this header: taps in order; inside a tap the input
// channels in chunks of 16, one MFMA per chunk.  Inside the MFMA lane half h supplies channels c + 8h .. c + 8h + 7 (one 16-byte
// load from a channels-last row) and the instruction adds the chunk's 16 products -- each exact in fp32, as a product of two fp16
// values is -- onto the accumulator in the hardware's own fixed order, which depends on nothing but the instruction.  The sum
// starts at zero (the kernels declare `f32x16 acc[MT][NT] = {}`); bias and everything after it belong to the caller's epilogue.
// No split-K and no float atomics, so results are bit-identical across batch sizes, clip positions and launch modes.
//
// The C/D register map is that of the 32x32 fp32 shape (column = lane & 31, row of register i = f32_cd_row(i, h)), so the
// epilogues of rva_mfma_f32.h (f32x16, f32_cd_row, f32_tile_sum) are used as they are.
#pragma once

#include "rva_mfma_f32.h"

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

// One chunk of 16 channels.  a[mt] + ao / b[nt] + bo = the lane's row of tile mt / nt at the chunk's first channel, already
// advanced by 8 h (16-byte aligned); a row whose flag is false reads nothing and contributes zeros.
template <int MT, int NT>
__device__ __forceinline__ void f16_chunk(f32x16 (&acc)[MT][NT], const _Float16 *const (&a)[MT], const bool (&av)[MT], size_t ao,
                                          const _Float16 *const (&b)[NT], size_t bo)
{
    f16x8 fa[MT], fb[NT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) fa[mt] = av[mt] ? *reinterpret_cast<const f16x8 *>(a[mt] + ao) : f16x8{};
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) fb[nt] = *reinterpret_cast<const f16x8 *>(b[nt] + bo);
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[mt], fb[nt], acc[mt][nt], 0, 0, 0);
}

// The tap loop of the fp16 clip plan: KT x 3 x 3 taps (kt, ky, kx) in order, pad 1, over a channels-last fp16 volume
// [Ti][Hi][Wi][CIN].  Position mt of the lane = (pt, py, px)[mt], computed only where pv[mt]; `w` = [32 NT][9 KT][CIN] fp16 weights
// of the wave's output channels.  Adds onto acc.
template <int CIN, int KT, int MT, int NT>
__device__ __forceinline__ void f16_conv_taps(f32x16 (&acc)[MT][NT], const _Float16 *in, const _Float16 *w, const int (&pt)[MT],
                                              const int (&py)[MT], const int (&px)[MT], const bool (&pv)[MT], int Ti, int Hi, int Wi)
{
    constexpr int CK = 16, TAPS = 9 * KT;
    static_assert(CIN % CK == 0, "whole chunks of 16 channels");
    const int r = threadIdx.x & 31, h = (threadIdx.x >> 5) & 1;
    for (int tap = 0; tap < TAPS; ++tap) {
        const int kt = tap / 9, ky = (tap / 3) % 3, kx = tap % 3;
        const _Float16 *arow[MT];
        bool av[MT];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            const int it = pt[mt] + kt - KT / 2, iy = py[mt] + ky - 1, ix = px[mt] + kx - 1;
            av[mt] = pv[mt] && (unsigned)it < (unsigned)Ti && (unsigned)iy < (unsigned)Hi && (unsigned)ix < (unsigned)Wi;
            arow[mt] = in + (((size_t)(av[mt] ? it : 0) * Hi + (av[mt] ? iy : 0)) * Wi + (av[mt] ? ix : 0)) * CIN + (CK / 2) * h;
        }
        const _Float16 *brow[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) brow[nt] = w + ((size_t)(nt * 32 + r) * TAPS + tap) * CIN + (CK / 2) * h;
#pragma unroll
        for (int c = 0; c < CIN; c += CK) f16_chunk<MT, NT>(acc, arow, av, c, brow, c);
    }
}

// f16_conv_taps for a 256-thread block whose four waves share the same 32 NT = 128 output channels: the weights go through LDS
// once per block where f16_conv_taps has every wave load them itself.  A step is one tap x 64 input channels: its [128][64]
// weights (16 KB) are fetched into registers during the step before, written to the other of two LDS buffers after that step's
// MFMAs, and one __syncthreads per step orders both.  The 16-byte slot q of row `row` lives at slot q ^ ((row >> 1) & 7), which
// keeps the 16 rows that one ds_read_b128 lane group reads on 16 different bank positions of the 256-byte bank row.  Same
// reduction order as f16_conv_taps, so the two are bit-identical.  Every thread of the block must call it (it synchronises).
template <int CIN, int KT, int MT>
__device__ __forceinline__ void f16_conv_taps_wlds(f32x16 (&acc)[MT][4], const _Float16 *in, const _Float16 *w, const int (&pt)[MT],
                                                   const int (&py)[MT], const int (&px)[MT], const bool (&pv)[MT], int Ti, int Hi, int Wi)
{
    constexpr int NT = 4, KB = 64, TAPS = 9 * KT, NKB = CIN / KB, STEPS = TAPS * NKB, ROWS = 32 * NT;
    constexpr int PER = ROWS * (KB / 8) / 256;               // 16-byte slots a thread stages per step (4)
    static_assert(CIN % KB == 0, "whole steps of 64 channels");
    __shared__ __attribute__((aligned(16))) _Float16 wl[2][ROWS * KB];
    const int tid = threadIdx.x, r = tid & 31, h = (tid >> 5) & 1;
    const int swz = (r >> 1) & 7;                            // of rows nt * 32 + r, for every nt
    f16x8 st[PER];
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const int s = tid + 256 * j, row = s >> 3, q = s & 7;
        st[j] = *reinterpret_cast<const f16x8 *>(w + (size_t)row * TAPS * CIN + q * 8);
    }
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const int s = tid + 256 * j, row = s >> 3, q = s & 7;
        *reinterpret_cast<f16x8 *>(&wl[0][row * KB + ((q ^ ((row >> 1) & 7)) << 3)]) = st[j];
    }
    __syncthreads();
    for (int step = 0; step < STEPS; ++step) {
        const int tap = step / NKB, kb = step % NKB;
        const bool more = step + 1 < STEPS;
        if (more) {
            const int ntap = (step + 1) / NKB, nkb = (step + 1) % NKB;
#pragma unroll
            for (int j = 0; j < PER; ++j) {
                const int s = tid + 256 * j, row = s >> 3, q = s & 7;
                st[j] = *reinterpret_cast<const f16x8 *>(w + ((size_t)row * TAPS + ntap) * CIN + nkb * KB + q * 8);
            }
        }
        const int kt = tap / 9, ky = (tap / 3) % 3, kx = tap % 3;
        f16x8 fa[KB / 16][MT];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            const int it = pt[mt] + kt - KT / 2, iy = py[mt] + ky - 1, ix = px[mt] + kx - 1;
            const bool av = pv[mt] && (unsigned)it < (unsigned)Ti && (unsigned)iy < (unsigned)Hi && (unsigned)ix < (unsigned)Wi;
            const _Float16 *arow = in + (((size_t)(av ? it : 0) * Hi + (av ? iy : 0)) * Wi + (av ? ix : 0)) * CIN + kb * KB + 8 * h;
#pragma unroll
            for (int c = 0; c < KB / 16; ++c) fa[c][mt] = av ? *reinterpret_cast<const f16x8 *>(arow + 16 * c) : f16x8{};
        }
        const _Float16 *wb = wl[step & 1];
#pragma unroll
        for (int c = 0; c < KB / 16; ++c) {
            f16x8 fb[NT];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
                fb[nt] = *reinterpret_cast<const f16x8 *>(wb + (nt * 32 + r) * KB + (((2 * c + h) ^ swz) << 3));
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
                    acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[c][mt], fb[nt], acc[mt][nt], 0, 0, 0);
        }
        if (more) {
#pragma unroll
            for (int j = 0; j < PER; ++j) {
                const int s = tid + 256 * j, row = s >> 3, q = s & 7;
                *reinterpret_cast<f16x8 *>(&wl[(step + 1) & 1][row * KB + ((q ^ ((row >> 1) & 7)) << 3)]) = st[j];
            }
        }
        __syncthreads();
    }
}
