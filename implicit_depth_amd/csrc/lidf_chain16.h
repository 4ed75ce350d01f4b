// lidf_chain16.h — what the any-width decoder chain's two kernels share (lidf_chain16.hip: exact f32;
// lidf_chain16_h.hip: split f16): the request of a sub-tile's gathered rows and prefetched operands, and a wavefront's
// range of sub-tiles. (The shorthands, the leaky ReLU and the output activation: lidf_mma.h.)
#pragma once
#include "lidf_mma.h"

#define C16_XPRE 7   // layer-1 k-quads whose operands are requested with the gathered rows (E <= 112: all of them)

template <int G, int NT>
__device__ __forceinline__ void c16_fetch(const Chain16Args& a, const long long AN, const long long half0,
                                          f32x4 (&base)[4 * G][NT], f32x4 (&xpre)[C16_XPRE][NT]) {
    constexpr int T1 = 4 * G;
    const int lane = threadIdx.x & 63;
    const int j = lane & 15, g = lane >> 4;
#pragma unroll
    for (int s = 0; s < NT; ++s) {
        const long long r0 = (half0 + s) * 16 + j;
        const long long r = r0 < AN ? r0 : AN - 1;
        const float* vp = a.voxpart ? a.voxpart + (size_t)(a.vox ? a.vox[r] : 0) * (64 * G) + 4 * g : nullptr;
        const float* rp = a.raypart ? a.raypart + (size_t)(a.ray ? a.ray[r] : r) * (64 * G) + 4 * g : nullptr;
        const float* xp = a.X + (size_t)r * a.ldx + 4 * g;
#pragma unroll
        for (int kq = 0; kq < C16_XPRE; ++kq) {
            f32x4 x = {0.f, 0.f, 0.f, 0.f};
            if (kq < a.KQ) {
                const f32x4u v = *(const f32x4u*)(xp + 16 * kq);
                // columns beyond E: their weights are zero, the operands must be too (0 x NaN)
#pragma unroll
                for (int i = 0; i < 4; ++i) x[i] = 16 * kq + 4 * g + i < a.E ? v[i] : 0.f;
            }
            xpre[kq][s] = x;
        }
#pragma unroll
        for (int T = 0; T < T1; ++T) {
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (vp) v = *(const f32x4*)(vp + 16 * T);
            if (rp) {
                const f32x4 w = *(const f32x4*)(rp + 16 * T);
#pragma unroll
                for (int i = 0; i < 4; ++i) v[i] += w[i];
            }
            base[T][s] = v;
        }
    }
}

// A wavefront's range [t, te) of 16-row sub-tiles and the row count AN of the launch. SLOTS wavefronts per SIMD
// (wavefronts w and w + 4 of a workgroup share one), NT sub-tiles side by side per wavefront: a SIMD owns a balanced,
// contiguous range of sub-tiles, its wavefronts split it.
// Device-side row count (the any-width frame route: a.n is the capacity the grid was sized from, the lists start
// at row a.row0 of the counted array): rows = clamp(*n_dev - row0, 0, n). Every row index of the kernels is clamped
// to AN - 1, so no element of vox / ray / X at or beyond the count is dereferenced; a wavefront whose balanced
// range is empty (all of them when AN == 0) leaves before it touches the ring.
template <int SLOTS, int NT>
__device__ __forceinline__ void c16_range(const Chain16Args& a, long long& AN, long long& t, long long& te) {
    long long an = a.n;
    if (a.n_dev) {
        const long long m = (long long)*a.n_dev - a.row0;
        an = m < an ? (m > 0 ? m : 0) : an;
    }
    AN = an;
    const long long nhalf = (AN + 15) / 16;
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long long nw = (long long)gridDim.x * 4, wv = (long long)blockIdx.x * 4 + (w & 3);
    const long long per = nhalf / nw, rem = nhalf % nw;
    t = wv * per + (wv < rem ? wv : rem);
    te = t + per + (wv < rem ? 1 : 0);
    if (SLOTS > 1) {
        // (every wavefront's share but the last a multiple of NT: no odd sub-tile in the middle of the range)
        const long long slot = w >> 2, cnt = te - t;
        const long long chunk = ((cnt + SLOTS - 1) / SLOTS + NT - 1) / NT * NT;
        const long long t0 = t + slot * chunk;
        t = t0 < te ? t0 : te;
        te = t0 + chunk < te ? t0 + chunk : te;
    }
}
