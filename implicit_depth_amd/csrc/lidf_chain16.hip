// lidf_chain16.hip — the decoder chain of lidf_chain16.h (layout of the stream, the tiles and the registers: there) in
// exact f32 on v_mfma_f32_16x16x4_f32: the any-width entries (gf_dim 32 / 64 / 128) and the stage-2 decoder. Round 6:
// the layer-by-layer path of these widths (generic.py: one lidf_linear_kernel launch per layer and pass, every
// activation through HBM) ran the query at 0.21 (gf 32) / 0.45 (gf 128) of the f32 matrix peak on its own FLOP.
#include "lidf_launch.h"
#include "lidf_chain16.h"

// One input tile per step as it is: register r of the lane's quad is the B operand of k-step r, the two weight quads
// are the A operands of two output tiles.
struct C16F32 {
    static constexpr int TIN = 1, WQ = 2;
    template <int NT>
    struct Opnd { f32x4 x[NT]; };
    static constexpr int l1_quads(int G, int kq) { return lidf_chain16_l1_quads(G, kq); }
    template <int NT>
    static __device__ __forceinline__ void prep(Opnd<NT>& op, const int s, const f32x4 (&x)[1]) { op.x[s] = x[0]; }
    template <int NT>
    static __device__ __forceinline__ void mac(const f32x4 (&q)[2], const Opnd<NT>& op, f32x4* acc0, f32x4* acc1) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
#pragma unroll
            for (int s = 0; s < NT; ++s) acc0[s] = MFMA16(q[0][r], op.x[s][r], acc0[s]);
#pragma unroll
            for (int s = 0; s < NT; ++s) acc1[s] = MFMA16(q[1][r], op.x[s][r], acc1[s]);
        }
    }
};

#define C16_XPRE 7   // any-width entries: k-groups requested with the gathered rows (E <= 112: all of them)

template <int G, int SLOTS, int NT>
__global__ void __launch_bounds__(256 * SLOTS) lidf_chain16_kernel(Chain16Args a) {
    c16_kernel<C16F32, G, SLOTS, NT, LIDF_CHAIN16_RING, C16_XPRE, false>(a);
}

// The stage-2 decoder: gf 64, two wavefronts per SIMD with one sub-tile each — the gaps of one instruction stream are
// filled by the other, at twice the weight-stream traffic per sub-tile (one wavefront walking two sub-tiles side by
// side, 256 + 78 registers, measured slower; a ring of 16 quads measured no faster than 8). embed(pos) of the shipped
// multires 8 .. 10 is four k-groups: all prefetched; dense tables.
__global__ void __launch_bounds__(512) lidf_ief16_kernel(Chain16Args a) {
    c16_kernel<C16F32, 4, 2, 1, LIDF_CHAIN16_RING, 4, true>(a);
}

// The one-row voxpart table of a chain launch whose layer 1 has no per-voxel columns, and the bias of the table
// launches that have them: out[f] = b1[f] + W1[f, enc columns] . benc (the IEF's constant; an IMNet's row is b1).
__global__ void __launch_bounds__(256) lidf_chain16_bias_row_kernel(const float* __restrict__ b1,
                                                                    const float* __restrict__ w1enc, int ld1,
                                                                    const float* __restrict__ benc, int nout,
                                                                    float* __restrict__ out) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= nout) return;
    float c = 0.f;
    for (int j = 0; j < 16; ++j) c = fmaf(w1enc[(size_t)f * ld1 + j], benc[j], c);
    out[f] = b1[f] + c;
}

extern "C" hipError_t lidf_launch_chain16_bias_row(const float* b1, const float* w1enc, int ld1, const float* benc,
                                                   int nout, float* out, hipStream_t st) {
    if (nout <= 0) return hipSuccess;
    hipLaunchKernelGGL(lidf_chain16_bias_row_kernel, dim3((unsigned)((nout + 255) / 256)), dim3(256), 0, st, b1,
                       w1enc, ld1, benc, nout, out);
    return hipGetLastError();
}

extern "C" hipError_t lidf_launch_chain16(int gf, const Chain16Args& a, int cus, hipStream_t st) {
    unsigned g;
    const hipError_t e = c16_grid(a, cus, g);
    if (e != hipSuccess || !g) return e;
    // gf 32: two wavefronts per SIMD, two sub-tiles each (64 + 32 + 16 accumulator registers per pair of sub-tiles);
    // gf 64: two wavefronts, one sub-tile each (the stage-2 decoder's configuration); gf 128: one wavefront, one
    // sub-tile (128 + 64 + 32 accumulator registers, the 512-register budget of a lone wavefront)
    switch (gf) {
        // (gf 32 at other occupancies — two wavefronts x one sub-tile, four x one, one x two — measured the same or
        // slower, docs/history.md section 13; those instantiations are not shipped)
        case 32: hipLaunchKernelGGL((lidf_chain16_kernel<2, 2, 2>), dim3(g), dim3(512), 0, st, a); break;
        case 64: hipLaunchKernelGGL((lidf_chain16_kernel<4, 2, 1>), dim3(g), dim3(512), 0, st, a); break;
        case 128: hipLaunchKernelGGL((lidf_chain16_kernel<8, 1, 1>), dim3(g), dim3(256), 0, st, a); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

extern "C" hipError_t lidf_launch_chain16_stage2(const Chain16Args& a, int cus, hipStream_t st) {
    unsigned g;
    const hipError_t e = c16_grid(a, cus, g);
    if (e != hipSuccess || !g) return e;
    if (!a.vox || !a.voxpart || !a.raypart || a.ray) return hipErrorInvalidValue;   // the dense form
    hipLaunchKernelGGL(lidf_ief16_kernel, dim3(g), dim3(512), 0, st, a);
    return hipGetLastError();
}
