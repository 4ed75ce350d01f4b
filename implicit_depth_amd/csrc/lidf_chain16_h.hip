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
// Stream (chain16h_stream_value in lidf_points.hip), 1 KiB quads consumed in order through a ring of R =
// lidf_chain16h_ring(G) quads:
//   layer 1: for kp < KP = ceil(KQ / 2), To < T1: the quad of high pieces, then the quad of low pieces, of
//            W1[16 To + j][c0 + 32 kp + 16 t + 4 g + 0..3], t = 0, 1 (0 beyond E)
//   pass:    the sections of lidf_chain16.hip's stream (f32 bias quads of layer 2; a f32 u quad in front of every fourth
//            input tile; f32 bias quads of layer 3; padding to a multiple of R), the weights per input-tile pair
//            (T, T + 1) and output tile To as a quad of high and a quad of low pieces of
//            W[16 To + j][16 (T + t) + 4 g + 0..3] — 4 bytes per weight as in the f32 stream.
// aux: w4 [gf] | b4 [1], f32.
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

template <int G, int NT, int RING>
__device__ __forceinline__ void c16h_tiles(const Chain16Args& a, const long long AN, const long long half0,
                                           const __amdgpu_buffer_rsrc_t srs, const int vq, f32x4 (&ring)[RING],
                                           int& pos, f32x4 (&base)[4 * G][NT], f32x4 (&xpre)[C16_XPRE][NT]) {
    constexpr int T1 = 4 * G, T2 = 2 * G, T3 = G;
    constexpr int NB2 = (T2 + 3) / 4, NB3 = (T3 + 3) / 4;
    constexpr int RAWQ = NB2 + T1 * T2 + T1 / 4 + NB3 + T2 * T3;
    constexpr int PASSQ = (RAWQ + RING - 1) / RING * RING;
    static_assert((2 * T1) % RING == 0 && RING % 4 == 0, "every layer-1 k-group pair must start on ring slot 0");
    static_assert(C16_XPRE == 7, "the prefetched k-groups are paired below as (0, 1) (2, 3) (4, 5) (6, the eighth)");
    const int lane = threadIdx.x & 63;
    const int j = lane & 15, g = lane >> 4;
    const int KP = (a.KQ + 1) / 2;
    const int l1_bytes = KP * 2 * T1 * 1024;
    // k-group kq = columns 16 kq + 4 g + {0..3} of the lane's rows, requested here (zero at or beyond E, and no load
    // of a group at or beyond KQ: the buffer is readable up to column 16 KQ only)
    auto x_group = [&](const int kq, f32x4 (&x)[NT]) {
#pragma unroll
        for (int s = 0; s < NT; ++s) {
            x[s] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (kq < a.KQ) {
                const long long r0 = (half0 + s) * 16 + j;
                const f32x4u v = *(const f32x4u*)(a.X + (size_t)(r0 < AN ? r0 : AN - 1) * a.ldx + 16 * kq + 4 * g);
#pragma unroll
                for (int i = 0; i < 4; ++i) x[s][i] = 16 * kq + 4 * g + i < a.E ? v[i] : 0.f;
            }
        }
    };
    f32x4 x7[NT];   // the eighth k-group (112 < E <= 128) is the partner of the last prefetched one
    x_group(C16_XPRE, x7);
    // ---- layer 1 on the per-row columns, a pair of k-groups per step
    auto l1_step = [&](const f32x4 (&xa)[NT], const f32x4 (&xb)[NT]) {
        h8 xh[NT], xl[NT];
#pragma unroll
        for (int s = 0; s < NT; ++s) c16h_split8(xa[s], xb[s], xh[s], xl[s]);
#pragma unroll
        for (int To = 0; To < T1; To += 2) {
            f32x4 q[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                q[u] = ring[(2 * To + u) % RING];
                ring[(2 * To + u) % RING] = LDQ(srs, vq, pos);   // refill RING quads ahead: ONE running position
                pos += 1024;
            }
            c16h_mac<NT>(q, xh, xl, base[To], base[To + 1]);
            SCHED_FENCE();
        }
    };
#pragma unroll
    for (int kp = 0; kp < (C16_XPRE + 1) / 2; ++kp) {
        if (kp < KP) {
            f32x4 xa[NT], xb[NT];
#pragma unroll
            for (int s = 0; s < NT; ++s) {
                xa[s] = xpre[2 * kp][s];
                xb[s] = 2 * kp + 1 < C16_XPRE ? xpre[(2 * kp + 1) % C16_XPRE][s] : x7[s];
            }
            l1_step(xa, xb);
        }
    }
    for (int kp = (C16_XPRE + 1) / 2; kp < KP; ++kp) {   // wider operands: requested here
        f32x4 xa[NT], xb[NT];
        x_group(2 * kp, xa);
        x_group(2 * kp + 1, xb);
        l1_step(xa, xb);
    }
    // ---- passes
    float val[NT];
#pragma unroll
    for (int s = 0; s < NT; ++s) val[s] = a.init;
    f32x4 w4v[T3];
#pragma unroll
    for (int T = 0; T < T3; ++T) w4v[T] = *(const f32x4*)(a.aux + 16 * T + 4 * g);
    const float b4 = a.aux[16 * G];
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    for (int pass = 0; pass < a.npass; ++pass) {
        // after this pass the stream continues with the same pass section (another pass) or with layer 1 of the next
        // tile (for a wavefront's last tile the loads are harmless re-reads)
        const bool last = pass + 1 == a.npass;
        const int wrap = last ? 0 : l1_bytes;
        int n = 0;   // quad index inside the pass section (compile-time through the unrolled loops)
#define C16H_NEXT(dst)                                                 \
    do {                                                               \
        dst = ring[n % RING];                                          \
        if (n + RING == PASSQ) pos = wrap;                             \
        ring[n % RING] = LDQ(srs, vq, pos);                            \
        pos += 1024;                                                   \
        ++n;                                                           \
    } while (0)
        f32x4 acc2[T2][NT];
#pragma unroll
        for (int qb = 0; qb < NB2; ++qb) {   // the bias quads of layer 2: acc = b2 x 1 (f32, exact)
            f32x4 bq;
            C16H_NEXT(bq);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (4 * qb + r < T2) {
#pragma unroll
                    for (int s = 0; s < NT; ++s) acc2[4 * qb + r][s] = MFMA16(bq[r], 1.f, zero4);
                }
            }
        }
        f32x4 uq = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int T = 0; T < T1; T += 2) {
            if (T % 4 == 0) C16H_NEXT(uq);
            h8 hh[NT], hl[NT];
#pragma unroll
            for (int s = 0; s < NT; ++s) {
                f32x4 h0 = MFMA16(uq[T % 4], val[s], base[T][s]);   // base + u * offset (group 0), f32
                f32x4 h1 = MFMA16(uq[T % 4 + 1], val[s], base[T + 1][s]);
                lrelu4(h0);
                lrelu4(h1);
                c16h_split8(h0, h1, hh[s], hl[s]);
            }
#pragma unroll
            for (int To = 0; To < T2; To += 2) {
                f32x4 q[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) C16H_NEXT(q[u]);
                c16h_mac<NT>(q, hh, hl, acc2[To], acc2[To + 1]);
                SCHED_FENCE();
            }
        }
        f32x4 acc3[T3][NT];
#pragma unroll
        for (int qb = 0; qb < NB3; ++qb) {   // the bias quads of layer 3
            f32x4 bq;
            C16H_NEXT(bq);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (4 * qb + r < T3) {
#pragma unroll
                    for (int s = 0; s < NT; ++s) acc3[4 * qb + r][s] = MFMA16(bq[r], 1.f, zero4);
                }
            }
        }
#pragma unroll
        for (int T = 0; T < T2; T += 2) {
            h8 hh[NT], hl[NT];
#pragma unroll
            for (int s = 0; s < NT; ++s) {
                lrelu4(acc2[T][s]);
                lrelu4(acc2[T + 1][s]);
                c16h_split8(acc2[T][s], acc2[T + 1][s], hh[s], hl[s]);
            }
#pragma unroll
            for (int To = 0; To < T3; To += 2) {
                f32x4 q[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) C16H_NEXT(q[u]);
                c16h_mac<NT>(q, hh, hl, acc3[To], acc3[To + 1]);
                SCHED_FENCE();
            }
        }
#pragma unroll
        for (int k = 0; k < PASSQ - RAWQ; ++k) {   // the padding quads: keep the ring in phase
            f32x4 unused;
            C16H_NEXT(unused);
            (void)unused;
        }
#undef C16H_NEXT
        // layer 4 (gf -> 1), f32: the lane's 4 G features, then the four groups of a row
#pragma unroll
        for (int s = 0; s < NT; ++s) {
            float y = 0.f;
#pragma unroll
            for (int T = 0; T < T3; ++T) {
                lrelu4(acc3[T][s]);
                const f32x4 w = w4v[T];
#pragma unroll
                for (int r = 0; r < 4; ++r) y += w[r] * acc3[T][s][r];
            }
            y += __shfl_xor(y, 16);
            y += __shfl_xor(y, 32);
            val[s] += y + b4;
        }
    }
#pragma unroll
    for (int s = 0; s < NT; ++s) {
        const long long r = (half0 + s) * 16 + j;
        if (r < AN && g == 0) a.out[r] = out_act(val[s], a.sigmoid);
    }
}

// SLOTS wavefronts per SIMD, NT sub-tiles side by side per wavefront (c16_range), RING weight quads in flight per
// wavefront (lidf_chain16h_ring(G): the packer pads the pass section to it).
template <int G, int SLOTS, int NT, int RING>
__global__ void __launch_bounds__(256 * SLOTS) lidf_chain16h_kernel(Chain16Args a) {
    constexpr int T1 = 4 * G, T2 = 2 * G, T3 = G;
    constexpr int PASSQ = ((T2 + 3) / 4 + T1 * T2 + T1 / 4 + (T3 + 3) / 4 + T2 * T3 + RING - 1) / RING * RING;
    long long AN, t, te;
    c16_range<SLOTS, NT>(a, AN, t, te);
    const int lane = threadIdx.x & 63;
    if (t >= te) return;
    const int total_bytes = ((a.KQ + 1) / 2 * 2 * T1 + PASSQ) * 1024;
    const __amdgpu_buffer_rsrc_t srs = __builtin_amdgcn_make_buffer_rsrc((void*)a.stream, 0, total_bytes, 0x00020000);
    const int vq = lane * 16;
    f32x4 ring[RING];
#pragma unroll
    for (int i = 0; i < RING; ++i) ring[i] = LDQ(srs, vq, i * 1024);
    int pos = RING * 1024;   // byte offset of the next quad to request
    if (NT == 2) {
        f32x4 base[T1][2], xpre[C16_XPRE][2];
        while (te - t >= 2) {
            c16_fetch<G, 2>(a, AN, t, base, xpre);
            c16h_tiles<G, 2, RING>(a, AN, t, srs, vq, ring, pos, base, xpre);
            t += 2;
        }
    }
    {
        f32x4 base[T1][1], xpre[C16_XPRE][1];
        for (; t < te; ++t) {
            c16_fetch<G, 1>(a, AN, t, base, xpre);
            c16h_tiles<G, 1, RING>(a, AN, t, srs, vq, ring, pos, base, xpre);
        }
    }
}

extern "C" hipError_t lidf_launch_chain16h(int gf, const Chain16Args& a, int cus, hipStream_t st) {
    if (a.n <= 0) return hipSuccess;
    if (a.KQ < 1 || a.npass < 1 || !a.X || !a.out) return hipErrorInvalidValue;
    const long long nhalf = (a.n + 15) / 16;
    long long g = (nhalf + 3) / 4;
    if (g > cus) g = cus;
    // gf 32 and 128: the occupancies of lidf_launch_chain16 (the accumulator sets are the same). gf 64: ONE wavefront
    // per SIMD with two sub-tiles instead of two with one — every weight quad feeds twice the rows, measured faster
    // on 4.9 M rows. The ring depths are lidf_chain16h_ring's.
    switch (gf) {
        case 32: hipLaunchKernelGGL((lidf_chain16h_kernel<2, 2, 2, 8>), dim3((unsigned)g), dim3(512), 0, st, a); break;
        case 64: hipLaunchKernelGGL((lidf_chain16h_kernel<4, 1, 2, 16>), dim3((unsigned)g), dim3(256), 0, st, a); break;
        case 128: hipLaunchKernelGGL((lidf_chain16h_kernel<8, 1, 1, 16>), dim3((unsigned)g), dim3(256), 0, st, a); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
