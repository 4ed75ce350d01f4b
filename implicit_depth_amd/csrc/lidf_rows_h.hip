// lidf_rows_h.hip — IMNet / IEF on materialised [n, D] rows with split-f16 matrix instructions
// (gfx950 only): the decoder boundary of the reference (models/pipeline.py:434-435) at the
// arithmetic of lidf_points_h.hip (w*x ~= wh*xh + wh*xl + wl*xh, f32 accumulation).
//
// Layer 1 is k-outer over the D input columns: per k-step of 16 columns every lane splits its 8
// row values into f16 pieces (the rows stream from HBM in double-buffered bursts of 8 k-steps),
// and all 8 output tiles accumulate (the 128-register pre-activation `base` is held for the IEF
// iterations, as in lidf_points.hip). Layers 2-4 are the k-outer chained pass: each H1 / H2 tile
// is consumed by all output tiles as soon as it has been produced. One wavefront per SIMD; the
// weight stream reaches the four wavefronts of a workgroup through the feed of lidf_split32.h, which
// also holds the section's tail, the steps of layers 2 to 4 and the packer.
//
// Stream per decoder: [layer 1: NKS k-steps x (8 tiles x (hi, lo))] [pass: 176 quads, RowsH::desc()].
#include "lidf_launch.h"
#include "lidf_mma.h"
#include "lidf_split32.h"

// ------------------------------------------------------------------------------------------------
// The kernel's policy (lidf_split32.h): its feed, the order of the pass section, its layer-1 quads
// ------------------------------------------------------------------------------------------------
struct RowsH {
    static constexpr int PASS = 176, RING = 4;
    // the staged chunk is published and the barrier stands at mid-chunk, behind a drained LDS queue
    static constexpr int PUBLISH_Q = 8, BARRIER_Q = 8, BARRIER_LGKM = 0;
    static constexpr bool L1_PREFIX = true, TILE_COUNTER = false;

    __host__ __device__ static constexpr QD desc(int s) {
        if (s < 4) return {K_B2, s, 0, 0, 0, 0};
        if (s == 4) return {K_U, 0, 0, 0, 0, 0};
        s -= 5;
        if (s < 7 * 17) {
            const int T = s / 17, r = s % 17;
            if (r == 0) return {K_U, 0, T + 1, 0, 0, 0};  // u of the NEXT tile, one segment early
            return l2_desc(T, r - 1);
        }
        return tail_desc(s - 7 * 17);
    }

    // layer 1, k-step ks: operand column 16ks + 8*half + i; column D carries b1 (+ the IEF constant)
    __device__ static _Float16 l1_prefix_value(const NetW& n, const L1Map& m, const int quad, const int half,
                                               const int o, const int i) {
        const int ks = quad / 16, r = quad % 16, t = r >> 1, part = r & 1;
        const int x = 16 * ks + 8 * half + i, out = 32 * t + o;
        float w = 0.f;
        if (x < m.D) {
            const int colw = x < m.n0 ? m.c0 + x : m.c1 + (x - m.n0);
            w = n.w1[(size_t)out * n.ld1 + colw];
        } else if (x == m.D && m.add_bias) {
            // (the terms join b1 one at a time: b1 + ief_c() would round in another order)
            w = n.b1[out];
            if (n.is_ief)
                for (int j = 0; j < 16; ++j) w += n.w1[(size_t)out * n.ld1 + n.dcore + j] * n.benc[j];
        }
        return hpiece(w, part);
    }
    // K_U: (uh, uh, ul) against (vh, vl, vh)
    __device__ static _Float16 l1_value(const NetW& n, const L1Map&, const QD d, const int half, const int o,
                                        const int i) {
        if (half != 0 || i >= 3 || !n.is_ief) return (_Float16)0.f;
        return hpiece(ief_u(n, 32 * d.T + o), i == 2 ? 1 : 0);
    }
};
static_assert(section_fits<RowsH>(5 + 7 * 17), "section size");

// One decoder pass on the 32 points of this wavefront (see lidf_points.hip:decoder_pass):
//   H1 = lrelu(base + u*val);  H2 = lrelu(W2 H1 + b2);  H3 = lrelu(W3 H2 + b3);  y = w4.H3 + b4
__device__ __forceinline__ float decoder_pass_h(Feed<RowsH>& f, const FeedCfg& c, f32x4* sb,
                                                const f32x16 (&base)[8], const float val,
                                                const int h, const float* __restrict__ ax) {
    const f32x4 onesB = ones_operand(h);
    f32x4 offB = {0.f, 0.f, 0.f, 0.f};
    if (!h) {
        const _Float16 vh = (_Float16)val;
        const _Float16 vl = (_Float16)(val - (float)vh);
        offB[0] = pack2(vh, vl);
        offB[1] = pack2(vh, (_Float16)0.f);
    }
    f32x16 pre;
    f32x4 bh[2][2], bl[2][2];      // split H1 tile, [parity of T][k-sub-step]
    TAIL32_STATE;               // layers 2 to 4
#pragma unroll
    for (int s = 0; s < RowsH::PASS; ++s) {
        const QD d = RowsH::desc(s);
        const f32x4 A = feed_take(f, c, sb, s % CH_QUADS);
        if (d.kind == K_U) {
            pre = MFMAH(A, offB, base[d.T]);
            if (d.T == 0) prep_pairs(0, 8, pre, bh[0], bl[0]);
        } else {
            const int par = d.T & 1;
            tail_step(TAIL32_ARGS, d, A, onesB, bh[par], bl[par]);
            // split pair j of the next H1 tile behind the matrix instructions of a high-piece step
            if (d.kind == K_L2 && !d.lo && d.T < 7) prep_pairs(d.j, d.j + 1, pre, bh[par ^ 1], bl[par ^ 1]);
            if (d.kind == K_B3 && d.t == 0) {
                // operands of layer 4, fetched here so that their latency hides behind layer 3
                tail_load_w4(w4, ax, h, 0, 8);
                b4 = ax[64];
            }
        }
        SCHED_FENCE();
    }
    return tail_finish(TAIL32_ARGS, b4);
}

#define XBURST 4   // k-steps of row operands per burst

__global__ void __launch_bounds__(256) lidf_rows_h_kernel(PointsArgs a) {
    __shared__ f32x4 sb[NBUF * CH_ELEMS];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int h = lane >> 5;
    const int col = lane & 31;

    const FeedCfg c = feed_cfg(a, lane, wave);
    const int nks = c.nk1;

    const long long AN = a.n_dev ? (long long)*a.n_dev : a.n;   // device-side count (the frame path)
    const long long ntile = (AN + 127) / 128;
    const long long per = ntile / gridDim.x, rem = ntile % gridDim.x;
    const long long tb = blockIdx.x * per + (blockIdx.x < rem ? blockIdx.x : rem);
    const long long te_ = tb + per + (blockIdx.x < rem ? 1 : 0);
    if (tb >= te_) return;

    Feed<RowsH> f;
    feed_start(f, c, sb);

    for (long long tile = tb; tile < te_; ++tile) {
        const long long p = tile * 128 + wave * 32 + col;
        const bool valid = p < AN;
        const long long pc = valid ? p : AN - 1;
        // this lane's operand columns in k-step ks: 16ks + 8h + {0..7}; column D = 1 (bias)
        const float* xrow = a.X + (size_t)pc * a.ldx + 8 * h;
        auto load_x = [&](int ks, f32x4 (&x)[2]) {
            const int x0 = 16 * ks + 8 * h;
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                if (x0 + 4 * q + 3 < a.D) {
                    const f32x4u v = *(const f32x4u*)(xrow + 16 * ks + 4 * q);
                    x[q] = f32x4{v[0], v[1], v[2], v[3]};
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int xc = x0 + 4 * q + i;
                        x[q][i] = xc < a.D ? xrow[16 * ks + 4 * q + i] : (xc == a.D ? 1.f : 0.f);
                    }
                }
            }
        };

        for (int net = 0; net < a.nets; ++net) {
            f32x16 base[8];
#pragma unroll
            for (int t = 0; t < 8; ++t) {
#pragma unroll
                for (int i = 0; i < 16; ++i) base[t][i] = 0.f;
            }
            // ---------------- layer 1 ----------------
            // The rows stream from HBM and VMEM loads return in order: the operands of XBURST
            // k-steps are fetched in one burst, the next burst while this one multiplies.
            f32x4 xa[XBURST][2], xn[XBURST][2];
#pragma unroll
            for (int i = 0; i < XBURST; ++i) {
                if (i < nks) load_x(i, xa[i]);
                else xa[i][0] = xa[i][1] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
            for (int k0 = 0; k0 < nks; k0 += XBURST) {
#pragma unroll
                for (int i = 0; i < XBURST; ++i) {
                    if (k0 + XBURST + i < nks) load_x(k0 + XBURST + i, xn[i]);
                    else xn[i][0] = xn[i][1] = f32x4{0.f, 0.f, 0.f, 0.f};
                }
                SCHED_FENCE();
#pragma unroll
                for (int i = 0; i < XBURST; ++i) {
                    if (k0 + i >= nks) break;
                    f32x4 ph, pl;
#pragma unroll
                    for (int w = 0; w < 4; ++w) {
                        float hi, lo;
                        split2(xa[i][w >> 1][2 * (w & 1)], xa[i][w >> 1][2 * (w & 1) + 1], hi, lo);
                        ph[w] = hi;
                        pl[w] = lo;
                    }
#pragma unroll
                    for (int q = 0; q < CH_QUADS; ++q) {
                        const int t = q >> 1;
                        const f32x4 A = feed_take(f, c, sb, q);
                        if (!(q & 1)) {
                            base[t] = MFMAH(A, ph, base[t]);
                            base[t] = MFMAH(A, pl, base[t]);
                        } else {
                            base[t] = MFMAH(A, ph, base[t]);
                        }
                        SCHED_FENCE();
                    }
                }
#pragma unroll
                for (int i = 0; i < XBURST; ++i) {
                    xa[i][0] = xn[i][0];
                    xa[i][1] = xn[i][1];
                }
            }

            if (a.out_base) {
                // layer-1-only use (the per-ray partial products of the query): [n, nets*256]
                if (valid) {
                    float* ob = a.out_base + ((size_t)p * a.nets + net) * 256 + 4 * h;
#pragma unroll
                    for (int t = 0; t < 8; ++t) {
#pragma unroll
                        for (int g = 0; g < 4; ++g) {
                            f32x4 v;
#pragma unroll
                            for (int i = 0; i < 4; ++i) v[i] = base[t][4 * g + i];
                            *(f32x4*)(ob + t * 32 + 8 * g) = v;
                        }
                    }
                }
                continue;
            }
            // ---------------- passes (1 for IMNet, n_iter for IEF) ----------------
            float val = a.init[net];
            const float* ax = a.aux + net * LIDF_AUX_FLOATS;
            const int npass = a.npass[net];
            for (int pass = 0; pass < npass; ++pass) val += decoder_pass_h(f, c, sb, base, val, h, ax);

            if (valid && h == 0 && a.out[net]) a.out[net][p] = out_act(val, a.sigmoid[net]);
        }
    }
}

// l1only: the stream holds the layer-1 sections only (npass must be 0 for every net)
extern "C" StreamLayout lidf_make_layout_rows_h(int nets, int D, int l1only) {
    StreamLayout s;
    s.nets = nets;
    s.mode = LIDF_MODE_FUSED_H;
    s.l1_quads = 16 * ((D + 1 + 15) / 16);
    s.net_quads = s.l1_quads + (l1only ? 0 : RowsH::PASS);
    s.total = nets * s.net_quads * 256;
    s.guard = nullptr;
    return s;
}

extern "C" hipError_t lidf_launch_pack_rows_h(const StreamLayout& lay, const NetW& n0, const NetW& n1,
                                              const L1Map& m, float* stream, float* aux,
                                              hipStream_t st) {
    return launch_pack_h<RowsH>(lay, n0, n1, m, stream, aux, st);
}

extern "C" hipError_t lidf_launch_rows_h(const PointsArgs& a, int grid, hipStream_t st) {
    if (a.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(lidf_rows_h_kernel, dim3(grid), dim3(256), 0, st, a);
    return hipGetLastError();
}
