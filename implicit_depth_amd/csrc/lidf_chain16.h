// lidf_chain16.h — the decoder chain on 16-row sub-tiles: IMNet / IEF (models/implicit_net.py:60-152, layers
// 4 gf -> 2 gf -> gf -> 1) as ONE register-chained launch per decoder. One tile body and one kernel body, in three
// uses: the any-width chain in exact f32 (lidf_chain16.hip: gf_dim 32 / 64 / 128 on v_mfma_f32_16x16x4_f32), its
// split-f16 form (lidf_chain16_h.hip: v_mfma_f32_16x16x32_f16 on f16 pieces) and the stage-2 decoder
// (RefineNet.get_pred_refine's offset_dec: lidf_ief16_kernel in lidf_chain16.hip, the f32 chain at gf 64 with dense
// tables). A precision policy P supplies what differs between the two arithmetics:
//   P::TIN            input tiles (layer 1: 16-column k-groups) one step consumes: 1 | 2
//   P::WQ             weight quads one step takes for its two output tiles: 2 | 4
//   P::Opnd<NT>       the prepared B operands of a step, for NT sub-tiles
//   P::prep           the lane's quads of the step's TIN input tiles -> operand (as is | c16h_split8)
//   P::mac            two output tiles += weights x operand (4 x MFMA16 per quad | c16h_mac)
//   P::l1_quads       the layer-1 section's length (lidf_device.h)
// (The shorthands, the leaky ReLU and the output activation: lidf_mma.h.)
//
// Why 16-row tiles: a frame's 76,800 rays are 2,400 wave-tiles of the 32 x 32 transposed-chain kernel (lidf_points.hip)
// over 1,024 SIMDs — 2.34 rounds of work in 3 rounds of time; the 16 x 16 x 4 instruction has the same rate on a tile
// of 16 rows, and a wavefront that walks 16-row sub-tiles (two side by side while it has two left, where the
// registers allow: every weight quad then feeds both) loses less to the partial round.
//
// Layer 1 arrives factorised: the per-row operand X [n, E] (the query: the 2 (3 + 6 L)
// position-embedding columns of a (ray, voxel) pair; stage 2: embed(pos); a materialised [n, D] input: all of it) is
// multiplied here, the columns that depend on the voxel / the ray alone arrive as gathered rows of two tables (voxpart
// carries b1 and the IEF's constant c = W1[:, enc] benc; in the any-width launches either gather may be absent).
//
// G = gf / 16. Accumulator tiles of 16 features x 16 rows: T1 = 4 G (layer 1), T2 = 2 G (layer 2), T3 = G (layer 3).
// Transposed chain: D[out feature][row] += A[out][k] B[k][row]. Lane l = (row j = l & 15, group g = l >> 4); register r
// of a tile T holds feature 16 T + 4 g + r of row j — the B operand of the next layer's k-step r of input tile T, so
// activations never leave the register file, and the matching A operand of the four k-steps is
// W[out][16 T + 4 g + 0..3]: four consecutive floats of nn.Linear's row.
//
// Stream (LIDF_MODE_CHAIN16, chain16_stream_value in lidf_points.hip; the split form's permutation of the weight
// quads: lidf_chain16_h.hip), 1 KiB quads = float4 per lane, consumed strictly in order through a ring of RING quads:
//   layer 1: for kq < KQ = ceil(E / 16), To < T1: lane l: W1[16 To + j][c0 + 16 kq + 4 g + 0..3] (0 beyond E)
//   pass:    ceil(T2 / 4) bias quads of layer 2 (component r of quad q = b2[16 (4 q + r) + j] in group 0, 0 elsewhere:
//            the accumulators start as bias x 1);
//            for T < T1: [T % 4 == 0: u quad — component r = u[16 (T + r) + j] in group 0: the IEF's rank-1 term
//            u * offset, implicit_net.py:135-139] then T2 quads W2[16 To + j][16 T + 4 g + 0..3];
//            ceil(T3 / 4) bias quads of layer 3; for T < T2: T3 quads W3[16 To + j][16 T + 4 g + ..];
//            padding to a multiple of the ring (lidf_chain16_pass_quads).
//   (biases as matrix steps, not loads: vector memory returns in order, a load of a bias vector at the head of a pass
//   waits behind the ring's requests and the ring behind it — measured 10 % of the stage-2 launch)
// aux: w4 [gf] | b4 [1] (read once per tile).
#pragma once
#include "lidf_mma.h"

// The gathered layer-1 terms (per-voxel row + per-ray row) and the first XPRE layer-1 k-groups of NT sub-tiles from
// half0 on. DENSE (stage 2): both tables and vox are there and row r's raypart row is row r — no tests, no index load.
template <int G, int NT, int XPRE, bool DENSE>
__device__ __forceinline__ void c16_fetch(const Chain16Args& a, const long long AN, const long long half0,
                                          f32x4 (&base)[4 * G][NT], f32x4 (&xpre)[XPRE][NT]) {
    constexpr int T1 = 4 * G;
    const int lane = threadIdx.x & 63;
    const int j = lane & 15, g = lane >> 4;
#pragma unroll
    for (int s = 0; s < NT; ++s) {
        const long long r0 = (half0 + s) * 16 + j;
        const long long r = r0 < AN ? r0 : AN - 1;
        const float* vp = DENSE ? a.voxpart + (size_t)a.vox[r] * (64 * G) + 4 * g
                          : a.voxpart ? a.voxpart + (size_t)(a.vox ? a.vox[r] : 0) * (64 * G) + 4 * g : nullptr;
        const float* rp = DENSE ? a.raypart + (size_t)r * (64 * G) + 4 * g
                          : a.raypart ? a.raypart + (size_t)(a.ray ? a.ray[r] : r) * (64 * G) + 4 * g : nullptr;
        const float* xp = a.X + (size_t)r * a.ldx + 4 * g;
#pragma unroll
        for (int kq = 0; kq < XPRE; ++kq) {
            f32x4 x = {0.f, 0.f, 0.f, 0.f};
            if (kq < a.KQ) {
                const f32x4u v = *(const f32x4u*)(xp + 16 * kq);
                // columns beyond E belong to other parts of the row (or were never written): their weights are zero,
                // the operands must be too (0 x NaN)
#pragma unroll
                for (int i = 0; i < 4; ++i) x[i] = 16 * kq + 4 * g + i < a.E ? v[i] : 0.f;
            }
            xpre[kq][s] = x;
        }
#pragma unroll
        for (int T = 0; T < T1; ++T) {
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (DENSE || vp) v = *(const f32x4*)(vp + 16 * T);
            if (DENSE || rp) {
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
// Device-side row count (the frame routes: a.n is the capacity the grid was sized from, the lists start at row
// a.row0 of the counted array): rows = clamp(*n_dev - row0, 0, n). Every row index of the kernels is clamped
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
    // (the wavefront index through readfirstlane: the compiler then knows the sub-tile range, the loop trip counts and
    // the running stream position to be wave-uniform — scalar registers, scalar adds)
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

// The oldest quad of the ring; its slot is refilled RING quads ahead. The stream is consumed strictly in order, so the
// position of the next request is ONE running (scalar) byte offset.
template <int RING>
__device__ __forceinline__ f32x4 c16_take(f32x4 (&ring)[RING], const int slot, const __amdgpu_buffer_rsrc_t srs,
                                          const int vq, int& pos) {
    const f32x4 q = ring[slot % RING];
    ring[slot % RING] = LDQ(srs, vq, pos);
    pos += 1024;
    return q;
}

// NT sub-tiles from half0 on; base / xpre arrive fetched.
template <class P, int G, int NT, int RING, int XPRE>
__device__ __forceinline__ void c16_tiles(const Chain16Args& a, const long long AN, const long long half0,
                                          const __amdgpu_buffer_rsrc_t srs, const int vq, f32x4 (&ring)[RING],
                                          int& pos, f32x4 (&base)[4 * G][NT], f32x4 (&xpre)[XPRE][NT]) {
    constexpr int T1 = 4 * G, T2 = 2 * G, T3 = G, TIN = P::TIN, WQ = P::WQ;
    constexpr int NB2 = (T2 + 3) / 4, NB3 = (T3 + 3) / 4;
    constexpr int PASSQ = lidf_chain16_pass_quads(G, RING), RAWQ = lidf_chain16_pass_quads(G, 1);
    static_assert((T1 * WQ / 2) % RING == 0 && RING % WQ == 0, "every layer-1 step must start on ring slot 0");
    typedef typename P::template Opnd<NT> Opnd;
    const int lane = threadIdx.x & 63;
    const int j = lane & 15, g = lane >> 4;
    const int steps = (a.KQ + TIN - 1) / TIN;
    const int l1_bytes = P::l1_quads(G, a.KQ) * 1024;
    // k-group kq = columns 16 kq + 4 g + {0..3} of the lane's rows, requested here (zero at or beyond E, and no load
    // of a group at or beyond KQ: the buffer is readable up to column 16 KQ only)
    auto x_group = [&](const int kq, f32x4 (&x)[NT]) __attribute__((always_inline)) {
#pragma unroll
        for (int s = 0; s < NT; ++s) {
            x[s] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (TIN == 1 || kq < a.KQ) {   // (one group per step: only groups below KQ are asked for)
                const long long r0 = (half0 + s) * 16 + j;
                const f32x4u v = *(const f32x4u*)(a.X + (size_t)(r0 < AN ? r0 : AN - 1) * a.ldx + 16 * kq + 4 * g);
#pragma unroll
                for (int i = 0; i < 4; ++i) x[s][i] = 16 * kq + 4 * g + i < a.E ? v[i] : 0.f;
            }
        }
    };
    f32x4 xlate[NT];   // TIN = 2 and an odd XPRE: the group behind the prefetched ones is the partner of the last one
    if (XPRE % TIN) x_group(XPRE, xlate);
    // ---- layer 1 on the per-row columns, TIN k-groups per step. Two output tiles per weight fetch: four (two)
    // independent accumulators between two matrix instructions on the same one — a 16 x 16 x 4 instruction issues in
    // 32 cycles, its result takes longer
    auto l1_step = [&](const f32x4 (&xin)[TIN][NT]) __attribute__((always_inline)) {
        Opnd op;
#pragma unroll
        for (int s = 0; s < NT; ++s) {
            f32x4 x[TIN];
#pragma unroll
            for (int i = 0; i < TIN; ++i) x[i] = xin[i][s];
            P::prep(op, s, x);
        }
#pragma unroll
        for (int To = 0; To < T1; To += 2) {
            f32x4 q[WQ];
#pragma unroll
            for (int u = 0; u < WQ; ++u) q[u] = c16_take(ring, WQ / 2 * To + u, srs, vq, pos);
            P::mac(q, op, base[To], base[To + 1]);
            SCHED_FENCE();
        }
    };
    // (every step starts on ring slot 0, so the prefetched groups unroll with their operands named at compile time)
#pragma unroll
    for (int i = 0; i < (XPRE + TIN - 1) / TIN; ++i) {
        if (i < steps) {
            f32x4 xin[TIN][NT];
#pragma unroll
            for (int u = 0; u < TIN; ++u) {
#pragma unroll
                for (int s = 0; s < NT; ++s) xin[u][s] = TIN * i + u < XPRE ? xpre[(TIN * i + u) % XPRE][s] : xlate[s];
            }
            l1_step(xin);
        }
    }
    for (int i = (XPRE + TIN - 1) / TIN; i < steps; ++i) {   // wider operands: requested here
        f32x4 xin[TIN][NT];
#pragma unroll
        for (int u = 0; u < TIN; ++u) x_group(TIN * i + u, xin[u]);
        l1_step(xin);
    }
    // ---- passes
    float val[NT];
#pragma unroll
    for (int s = 0; s < NT; ++s) val[s] = a.init;
    // layer 4's weights and bias: once per tile, before the matrix stream starts
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
        auto next = [&]() __attribute__((always_inline)) {
            if (n + RING == PASSQ) pos = wrap;
            return c16_take(ring, n++, srs, vq, pos);
        };
        // acc[t] = b[t] x 1 from the bias quads of a layer (f32, exact)
        auto bias = [&](f32x4 (*acc)[NT], const int tiles) __attribute__((always_inline)) {
#pragma unroll
            for (int qb = 0; qb < (tiles + 3) / 4; ++qb) {
                const f32x4 bq = next();
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    if (4 * qb + r < tiles) {
#pragma unroll
                        for (int s = 0; s < NT; ++s) acc[4 * qb + r][s] = MFMA16(bq[r], 1.f, zero4);
                    }
                }
            }
        };
        // acc (TO output tiles) += the next TO / 2 weight fetches x op
        auto layer_step = [&](f32x4 (*acc)[NT], const int TO, const Opnd& op) __attribute__((always_inline)) {
#pragma unroll
            for (int To = 0; To < TO; To += 2) {
                f32x4 q[WQ];
#pragma unroll
                for (int u = 0; u < WQ; ++u) q[u] = next();
                P::mac(q, op, acc[To], acc[To + 1]);
                SCHED_FENCE();
            }
        };
        f32x4 acc2[T2][NT];
        bias(acc2, T2);
        f32x4 uq = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int T = 0; T < T1; T += TIN) {
            if (T % 4 == 0) uq = next();
            Opnd op;
#pragma unroll
            for (int s = 0; s < NT; ++s) {
                f32x4 h[TIN];
#pragma unroll
                for (int i = 0; i < TIN; ++i)   // base + u * offset (u lives in group 0 only), f32
                    h[i] = MFMA16(uq[(T + i) % 4], val[s], base[T + i][s]);
#pragma unroll
                for (int i = 0; i < TIN; ++i) lrelu4(h[i]);
                P::prep(op, s, h);
            }
            layer_step(acc2, T2, op);
        }
        // (requesting the next tile's gathered rows here — base is dead in the last pass — was measured slower in the
        // stage-2 launch, 157 -> 167 us: vector memory returns in order, so ~70 gather requests in front of the weight
        // ring's loads stall the ring for their whole latency, in the middle of the matrix stream)
        f32x4 acc3[T3][NT];
        bias(acc3, T3);
#pragma unroll
        for (int T = 0; T < T2; T += TIN) {
            Opnd op;
#pragma unroll
            for (int s = 0; s < NT; ++s) {
                f32x4 h[TIN];
#pragma unroll
                for (int i = 0; i < TIN; ++i) {
                    lrelu4(acc2[T + i][s]);
                    h[i] = acc2[T + i][s];
                }
                P::prep(op, s, h);
            }
            layer_step(acc3, T3, op);
        }
#pragma unroll
        for (int k = 0; k < PASSQ - RAWQ; ++k) (void)next();   // the padding quads: keep the ring in phase
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

// The body of every chain kernel. SLOTS wavefronts per SIMD, NT sub-tiles side by side per wavefront while it has NT
// left, then one at a time (c16_range); RING weight quads in flight per wavefront (the packer pads the pass section
// to it); XPRE layer-1 k-groups requested with the gathered rows, the wider operands' other groups inside layer 1.
template <class P, int G, int SLOTS, int NT, int RING, int XPRE, bool DENSE>
__device__ __forceinline__ void c16_kernel(const Chain16Args& a) {
    constexpr int T1 = 4 * G;
    long long AN, t, te;
    c16_range<SLOTS, NT>(a, AN, t, te);
    const int lane = threadIdx.x & 63;
    if (t >= te) return;
    const int total_bytes = (P::l1_quads(G, a.KQ) + lidf_chain16_pass_quads(G, RING)) * 1024;
    const __amdgpu_buffer_rsrc_t srs = __builtin_amdgcn_make_buffer_rsrc((void*)a.stream, 0, total_bytes, 0x00020000);
    const int vq = lane * 16;
    f32x4 ring[RING];
#pragma unroll
    for (int i = 0; i < RING; ++i) ring[i] = LDQ(srs, vq, i * 1024);
    int pos = RING * 1024;   // byte offset of the next quad to request
    if (NT == 2) {
        f32x4 base[T1][2], xpre[XPRE][2];
        while (te - t >= 2) {
            c16_fetch<G, 2, XPRE, DENSE>(a, AN, t, base, xpre);
            c16_tiles<P, G, 2, RING, XPRE>(a, AN, t, srs, vq, ring, pos, base, xpre);
            t += 2;
        }
    }
    {
        f32x4 base[T1][1], xpre[XPRE][1];
        for (; t < te; ++t) {
            c16_fetch<G, 1, XPRE, DENSE>(a, AN, t, base, xpre);
            c16_tiles<P, G, 1, RING, XPRE>(a, AN, t, srs, vq, ring, pos, base, xpre);
        }
    }
}

// Host: the guards every chain launcher shares and the grid (a workgroup per compute unit at most, four sub-tiles —
// one per SIMD — at least). 0 blocks: nothing to launch, with the answer in the return value.
static inline hipError_t c16_grid(const Chain16Args& a, const int cus, unsigned& blocks) {
    blocks = 0;
    if (a.n <= 0) return hipSuccess;
    if (a.KQ < 1 || a.npass < 1 || !a.X || !a.out) return hipErrorInvalidValue;
    const long long nhalf = (a.n + 15) / 16;
    const long long g = (nhalf + 3) / 4;
    blocks = (unsigned)(g > cus ? cus : g);
    return hipSuccess;
}
