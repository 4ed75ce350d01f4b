// lidf_mma.h — what the matrix kernels' files share, one definition each: the matrix-instruction, scheduling-fence and
// buffer-load shorthands, the decoders' output activation and leaky ReLUs, and the pieces of the split-f16 arithmetic
// (w*x ~= wh*xh + wh*xl + wl*xh on f16 pieces with f32 accumulation; the kernels over lidf_split32.h, whose
// float64 twin is tests/split_f16_ref.py). Several of these are numerical contracts that the float64 tests pin.
#pragma once
#include "lidf_launch.h"

typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef _Float16 h2 __attribute__((ext_vector_type(2)));

#define MFMA(a, b, c) __builtin_amdgcn_mfma_f32_32x32x2f32((a), (b), (c), 0, 0, 0)
#define MFMA16(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)
#define MFMAH(a, b, c) \
    __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(h8, (a)), __builtin_bit_cast(h8, (b)), (c), 0, 0, 0)
#define MFMA32H(a, b, c) __builtin_amdgcn_mfma_f32_16x16x32_f16((a), (b), (c), 0, 0, 0)
#define SCHED_FENCE() __builtin_amdgcn_sched_barrier(0)
// Weight-stream loads go through a buffer descriptor: the (wave-uniform) stream position lives in
// an SGPR and the lane offset is one constant VGPR, so the unrolled layers need no per-load
// 64-bit address registers (with flat pointers hipcc materialises and spills hundreds of them).
#define LDQ(rs, voff, soff) \
    __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128((rs), (voff), (soff), 0))

// the weight stream of the split-f16 feed (lidf_split32.h) reaches the wavefronts through LDS in chunks
#define CH_QUADS 16
#define CH_ELEMS (CH_QUADS * 64)  // f32x4 elements per chunk buffer
#define NBUF 3

// ---- activations --------------------------------------------------------------------------------
// the decoders' output activation, implicit_net.py:93-96 / :148-151:
// max(min(y, 0.01 y + 0.99), 0.01 y) — identity on [0, 1], slope 0.01 outside — or the sigmoid
__device__ __forceinline__ float out_act(float y, int use_sigmoid) {
    if (use_sigmoid) return 1.f / (1.f + expf(-y));
    return fmaxf(fminf(y, y * 0.01f + 0.99f), y * 0.01f);
}

// leaky_relu(0.02) of one register
__device__ __forceinline__ float lrelu1(const float x) {
    const float t = x * 0.02f;
    float r;
    asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(x), "v"(t));
    return r;
}

// leaky_relu(0.02) on the four registers of a tile: packed multiplies + one v_med3_f32 per register —
// max(x, 0.02 x) = med3(x, 0.02 x, +inf). fmaxf would add a canonicalising v_max per input under the IEEE
// mode (on gfx950 every vector instruction of the wavefront delays its f32 matrix instructions); inline
// assembly instead hides the operands from the compiler's matrix-result hazard tracking (measured: wrong
// values).
__device__ __forceinline__ void lrelu4(f32x4& v) {
    const f32x4 t = v * 0.02f;
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = __builtin_amdgcn_fmed3f(v[i], t[i], __builtin_inff());
}

// ---- split-f16 pieces ---------------------------------------------------------------------------
// feature held by register r of a 32x32 result tile in half-wave `half`
__host__ __device__ constexpr int tile_feature(int r, int half) {
    return (r & 3) + 8 * (r >> 2) + 4 * half;
}

// piece `part` of w = hi + lo + rest (the packers; round to nearest, w - hi is exact in f32)
__device__ __forceinline__ _Float16 hpiece(float w, int part) {
    const _Float16 hi = (_Float16)w;
    if (part == 0) return hi;
    const float r = w - (float)hi;
    const _Float16 lo = (_Float16)r;
    if (part == 1) return lo;
    return (_Float16)(r - (float)lo);
}

// the IEF term of layer 1, W1[:, D:D+16] (wenc*off + benc) = u*off + c: row `out` of u and of c (the packers)
__device__ __forceinline__ float ief_u(const NetW& n, int out) {
    float acc = 0.f;
    for (int j = 0; j < 16; ++j) acc += n.w1[(size_t)out * n.ld1 + n.dcore + j] * n.wenc[j];
    return acc;
}
__device__ __forceinline__ float ief_c(const NetW& n, int out) {
    float acc = 0.f;
    for (int j = 0; j < 16; ++j) acc += n.w1[(size_t)out * n.ld1 + n.dcore + j] * n.benc[j];
    return acc;
}

// element e of the split-f16 packer's aux array, LIDF_AUX_FLOATS floats per net: w4 by (half, register) of the two
// layer-3 tiles, b4 at [64]. (The two nets by reference, selected per element: a NetW[2] copy indexed by a runtime
// value lives in scratch.)
__device__ __forceinline__ void pack_aux_h(const NetW& net0, const NetW& net1, const long long e, float* aux) {
    const int sec = (int)e / LIDF_AUX_FLOATS, i = (int)e % LIDF_AUX_FLOATS;
    const NetW& n = sec ? net1 : net0;
    float v = 0.f;
    if (i < 64) {
        const int half = i / 32, s = i % 32;
        v = n.w4[32 * (s >> 4) + tile_feature(s & 15, half)];
    } else if (i == 64) {
        v = n.b4[0];
    }
    aux[e] = v;
}

__device__ __forceinline__ float pack2(const _Float16 a, const _Float16 b) {
    h2 v;
    v[0] = a;
    v[1] = b;
    return __builtin_bit_cast(float, v);
}

// x -> one word holding (hi piece, lo piece) of x
__device__ __forceinline__ float split1(const float x) {
    const _Float16 hi = (_Float16)x;
    const _Float16 lo = (_Float16)(x - (float)hi);
    return pack2(hi, lo);
}

// (x0, x1) -> packed f16 high pieces (round to nearest) and packed f16 residuals. x - hi is exact
// in f32; v_fma_mix_f32 reads the f16 half directly (1 instruction per residual).
__device__ __forceinline__ void split2(const float x0, const float x1, float& hi, float& lo) {
    h2 hh;
    hh[0] = (_Float16)x0;
    hh[1] = (_Float16)x1;
    const float hw = __builtin_bit_cast(float, hh);
    float r0, r1;
    asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(r0) : "v"(hw), "v"(x0));
    asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]"
        : "=v"(r1)
        : "v"(hw), "v"(x1));
    h2 ll;
    ll[0] = (_Float16)r0;
    ll[1] = (_Float16)r1;
    hi = hw;
    lo = __builtin_bit_cast(float, ll);
}

// pairs [p0, p1) of a result tile: leaky-relu, split, store into the two k-sub-step fragments
// (p0, p1 are compile-time constants after unrolling)
__device__ __forceinline__ void prep_pairs(const int p0, const int p1, const f32x16& pre,
                                           f32x4 (&bh)[2], f32x4 (&bl)[2]) {
#pragma unroll
    for (int p = 0; p < 8; ++p) {
        if (p >= p0 && p < p1) {
            float hi, lo;
            split2(lrelu1(pre[2 * p]), lrelu1(pre[2 * p + 1]), hi, lo);
            bh[p >> 2][p & 3] = hi;
            bl[p >> 2][p & 3] = lo;
        }
    }
}
