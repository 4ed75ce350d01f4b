// lidf_chain16_h.hip — the split-f16 sibling of lidf_chain16.hip (precision "f16x3" at gf_dim 32 / 64 / 128): the
// same register-chained launch per decoder, the same Chain16Args, the same balanced split of 16-row sub-tiles over
// SIMDs and wavefronts, the same weight ring through buffer loads, the same clamping of row indices to AN - 1 and
// masking of operand columns at or beyond E. Every product of layers 1 (per-row columns), 2 and 3 is
//     wh * xh + wh * xl + wl * xh          (wl * xl dropped, f16 subnormal pieces kept)
// on v_mfma_f32_16x16x32_f16 with f32 accumulation: wh = f16(w), wl = f16(w - wh) come split from the packer
// (LIDF_MODE_CHAIN16_H), xh = f16(x), xl = f16(x - xh) are split in registers. The accumulator tile of a layer leaves
// lane l = (row j = l & 15, group g = l >> 4) with features 16 T + 4 g + 0..3 of row j in its four registers. The
// f16 instruction's B operand is k = 8 g + 0..7 of column j: the lane's quads of TWO input tiles (T, T + 1) side by
// side (k = 8 g + c: feature 4 g + (c & 3) of tile T + (c >> 2)), with the weight stream permuted the same way — ONE
// matrix instruction per piece product takes the two 16-feature input tiles the f32 form needs eight for, and no
// activation leaves the register file.
//
// What stays f32, on v_mfma_f32_16x16x4_f32 as in lidf_chain16.hip: the biases of layers 2 / 3 (b x 1 into a zero
// accumulator: exact) and the IEF's rank-1 term (base + u * offset, one rounding). The gathered voxpart / raypart rows
// are f32 and summed on the vector unit into the layer-1 accumulators; layer 4, the running offset and the output
// activation are f32 on the vector unit.
//
// Stream (chain16h_stream_value in lidf_points.hip): the sections of lidf_chain16.h's stream through a ring of R =
// lidf_chain16h_ring(G) quads; the bias, u and padding quads are f32 as there; the WEIGHT quads are permuted:
//   layer 1: for kp < KP = ceil(KQ / 2), To < T1: the quad of high pieces, then the quad of low pieces, of
//            W1[16 To + j][c0 + 32 kp + 16 t + 4 g + 0..3], t = 0, 1 (0 beyond E)
//   pass:    per input-tile pair (T, T + 1) and output tile To a quad of high and a quad of low pieces of
//            W[16 To + j][16 (T + t) + 4 g + 0..3] — 4 bytes per weight as in the f32 stream.
#include "lidf_launch.h"
#include "lidf_chain16.h"

// the lane's quads of two input tiles -> the f16 high pieces (round to nearest even) and the f16 residuals as the
// instruction's B operands; x - hi is exact in f32
__device__ __forceinline__ void c16h_split8(const f32x4& x0, const f32x4& x1, h8& hi, h8& lo) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const float x = i < 4 ? x0[i] : x1[i - 4];
        hi[i] = (_Float16)x;
        lo[i] = (_Float16)(x - (float)hi[i]);
    }
}

// acc0 / acc1 (two output tiles) += the three piece products of their weight quads q = {high 0, low 0, high 1, low 1}
// with the split operand of every sub-tile: piece-major, so that consecutive matrix instructions write different
// accumulators
template <int NT>
__device__ __forceinline__ void c16h_mac(const f32x4 (&q)[4], const h8 (&xh)[NT], const h8 (&xl)[NT], f32x4* acc0,
                                         f32x4* acc1) {
    const h8 wh[2] = {__builtin_bit_cast(h8, q[0]), __builtin_bit_cast(h8, q[2])};
    const h8 wl[2] = {__builtin_bit_cast(h8, q[1]), __builtin_bit_cast(h8, q[3])};
#pragma unroll
    for (int s = 0; s < NT; ++s) {
        acc0[s] = MFMA32H(wh[0], xh[s], acc0[s]);
        acc1[s] = MFMA32H(wh[1], xh[s], acc1[s]);
    }
#pragma unroll
    for (int s = 0; s < NT; ++s) {
        acc0[s] = MFMA32H(wh[0], xl[s], acc0[s]);
        acc1[s] = MFMA32H(wh[1], xl[s], acc1[s]);
    }
#pragma unroll
    for (int s = 0; s < NT; ++s) {
        acc0[s] = MFMA32H(wl[0], xh[s], acc0[s]);
        acc1[s] = MFMA32H(wl[1], xh[s], acc1[s]);
    }
}

// Two input tiles per step, split in registers; four weight quads = high and low pieces of two output tiles.
struct C16Split {
    static constexpr int TIN = 2, WQ = 4;
    template <int NT>
    struct Opnd { h8 hi[NT], lo[NT]; };
    static constexpr int l1_quads(int G, int kq) { return lidf_chain16h_l1_quads(G, kq); }
    template <int NT>
    static __device__ __forceinline__ void prep(Opnd<NT>& op, const int s, const f32x4 (&x)[2]) {
        c16h_split8(x[0], x[1], op.hi[s], op.lo[s]);
    }
    template <int NT>
    static __device__ __forceinline__ void mac(const f32x4 (&q)[4], const Opnd<NT>& op, f32x4* acc0, f32x4* acc1) {
        c16h_mac<NT>(q, op.hi, op.lo, acc0, acc1);
    }
};

// (seven prefetched k-groups pair as (0, 1) (2, 3) (4, 5) (6, the eighth): 112 < E <= 128 requests its last group with
// the tile's first step)
#define C16H_XPRE 7

template <int G, int SLOTS, int NT, int RING>
__global__ void __launch_bounds__(256 * SLOTS) lidf_chain16h_kernel(Chain16Args a) {
    c16_kernel<C16Split, G, SLOTS, NT, RING, C16H_XPRE, false>(a);
}

extern "C" hipError_t lidf_launch_chain16h(int gf, const Chain16Args& a, int cus, hipStream_t st) {
    unsigned g;
    const hipError_t e = c16_grid(a, cus, g);
    if (e != hipSuccess || !g) return e;
    // gf 32 and 128: the occupancies of lidf_launch_chain16 (the accumulator sets are the same). gf 64: ONE wavefront
    // per SIMD with two sub-tiles instead of two with one — every weight quad feeds twice the rows, measured faster
    // on 4.9 M rows. The ring depths are lidf_chain16h_ring's.
    switch (gf) {
        case 32: hipLaunchKernelGGL((lidf_chain16h_kernel<2, 2, 2, 8>), dim3(g), dim3(512), 0, st, a); break;
        case 64: hipLaunchKernelGGL((lidf_chain16h_kernel<4, 1, 2, 16>), dim3(g), dim3(256), 0, st, a); break;
        case 128: hipLaunchKernelGGL((lidf_chain16h_kernel<8, 1, 1, 16>), dim3(g), dim3(256), 0, st, a); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
