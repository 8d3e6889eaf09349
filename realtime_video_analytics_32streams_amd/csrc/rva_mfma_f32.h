// The one fp32 implicit-GEMM core on the exact fp32-input MFMA (v_mfma_f32_32x32x2_f32), included by rva_conv_f32.hip,
// rva_clip.hip and rva_clip3d.hip (device code only).  A wave owns MT x NT tiles of 32 GEMM rows (output positions) x 32 columns
// (output channels); lane & 31 = row of an A tile and column of a B tile, lane >> 5 = lane half h.
//
// THE reduction order of an output element, for every kernel built on this header: taps in order; inside a tap the input
// channels in chunks of CK; in a chunk MFMA step (q, e), q = 0 .. CK/8 - 1, e = 0 .. 3, takes channel c + 4q + e on lane half 0
// and then c + CK/2 + 4q + e on lane half 1.  The sum starts at zero (the kernels declare `f32x16 acc[MT][NT] = {}`: zeroing
// through a reference in a helper costs k_conv_f32<2,2> an AGPR round trip of the tile per tap); bias and everything after it
// belong to the caller's epilogue.  No split-K and no float atomics, so results are bit-identical across tile shapes, batch sizes and launch modes.
//
// C/D map of the 32x32 shapes: column = lane & 31, row of register i = f32_cd_row(i, h).
#pragma once

#include <hip/hip_runtime.h>

typedef float f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ int f32_cd_row(int i, int h) { return (i & 3) + 8 * (i >> 2) + 4 * h; }

__device__ __forceinline__ float f32_lane(const float4 &v, int e) { return e == 0 ? v.x : e == 1 ? v.y : e == 2 ? v.z : v.w; }

// One chunk of CK channels.  a[mt] + ao / b[nt] + bo = the lane's row of tile mt / nt at the chunk's first channel, already
// advanced by (CK / 2) * h; a row whose flag is false reads nothing and contributes zeros.
template <int MT, int NT, int CK>
__device__ __forceinline__ void f32_chunk(f32x16 (&acc)[MT][NT], const float *const (&a)[MT], const bool (&av)[MT], size_t ao,
                                          const float *const (&b)[NT], const bool (&bv)[NT], size_t bo)
{
    constexpr int NQ = CK / 8;                      // float4 loads per lane per operand per chunk
    float4 fa[MT][NQ], fb[NT][NQ];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int q = 0; q < NQ; ++q)
            fa[mt][q] = av[mt] ? *reinterpret_cast<const float4 *>(a[mt] + ao + 4 * q) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int q = 0; q < NQ; ++q)
            fb[nt][q] = bv[nt] ? *reinterpret_cast<const float4 *>(b[nt] + bo + 4 * q) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int q = 0; q < NQ; ++q)
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
                    acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(f32_lane(fa[mt][q], e), f32_lane(fb[nt][q], e), acc[mt][nt], 0, 0, 0);
}

// The tap loop of the clip plans: KT x 3 x 3 taps (kt, ky, kx) in order, pad 1, over a channels-last volume [Ti][Hi][Wi][CIN],
// CK = 32.  Position mt of the lane = (pt, py, px)[mt], computed only where pv[mt]; `w` = [32 NT][9 KT][CIN] weights of the
// wave's output channels.  KT = 1 with Ti = 1 and pt = 0 is a 2D 3x3 convolution.  Adds onto acc.
template <int CIN, int KT, int MT, int NT>
__device__ __forceinline__ void f32_conv_taps(f32x16 (&acc)[MT][NT], const float *in, const float *w, const int (&pt)[MT],
                                              const int (&py)[MT], const int (&px)[MT], const bool (&pv)[MT], int Ti, int Hi, int Wi)
{
    constexpr int CK = 32, TAPS = 9 * KT;
    const int r = threadIdx.x & 31, h = (threadIdx.x >> 5) & 1;
    bool bv[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) bv[nt] = true;
    for (int tap = 0; tap < TAPS; ++tap) {
        const int kt = tap / 9, ky = (tap / 3) % 3, kx = tap % 3;
        const float *arow[MT];
        bool av[MT];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            const int it = pt[mt] + kt - KT / 2, iy = py[mt] + ky - 1, ix = px[mt] + kx - 1;
            av[mt] = pv[mt] && (unsigned)it < (unsigned)Ti && (unsigned)iy < (unsigned)Hi && (unsigned)ix < (unsigned)Wi;
            arow[mt] = in + (((size_t)(av[mt] ? it : 0) * Hi + (av[mt] ? iy : 0)) * Wi + (av[mt] ? ix : 0)) * CIN + (CK / 2) * h;
        }
        const float *brow[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) brow[nt] = w + ((size_t)(nt * 32 + r) * TAPS + tap) * CIN + (CK / 2) * h;
#pragma unroll
        for (int c = 0; c < CIN; c += CK) f32_chunk<MT, NT, CK>(acc, arow, av, c, brow, bv, c);
    }
}

// The "bias + ReLU + per-channel tile sum" epilogue of a 256-thread block whose wave `wave` holds positions m0 .. m0 + 32 MT - 1
// of P: v = max(acc + bias, 0); per channel the sum over the wave's positions (mt, then i, in order, p >= P skipped), lane
// halves 0 + 1, then waves 0..3 from zero.  out[co] = the block's sum of channel co, co < 32 NT.
template <int MT, int NT>
__device__ __forceinline__ void f32_tile_sum(const f32x16 (&acc)[MT][NT], const float *bias, int m0, int P, float *out)
{
    __shared__ float red[4][2][32 * NT];
    const int r = threadIdx.x & 31, h = (threadIdx.x >> 5) & 1, wave = threadIdx.x >> 6;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int co = nt * 32 + r;
        const float b = bias[co];
        float s = 0.f;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int i = 0; i < 16; ++i)
                if (m0 + mt * 32 + f32_cd_row(i, h) < P) s = s + fmaxf(acc[mt][nt][i] + b, 0.f);
        red[wave][h][co] = s;
    }
    __syncthreads();
    if (threadIdx.x < 32 * NT) {
        const int co = threadIdx.x;
        float s = 0.f;
#pragma unroll
        for (int wv = 0; wv < 4; ++wv) s = s + (red[wv][0][co] + red[wv][1][co]);
        out[co] = s;
    }
}
