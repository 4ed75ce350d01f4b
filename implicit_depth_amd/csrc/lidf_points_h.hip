// lidf_points_h.hip — the fused per-point query with split-f16 matrix instructions (gfx950 only).
//
// Same computation and same register-chained, transposed formulation as lidf_points.hip (FUSED
// mode), but every f32 product  w*x  of layers 1-3 is evaluated as
//     w*x ~= wh*xh + wh*xl + wl*xh ,   w = wh + wl,  x = xh + xl   (f16 pieces, f32 accumulation)
// on v_mfma_f32_32x32x16_f16: three instructions of 32 cycles per 16 k instead of eight f32
// instructions of 64 cycles. The dropped wl*xl term is <= 2^-22 |w x|; against float64 the kernel
// is within 1.5 x (a float64 twin of these f16 pieces + the f32 oracle), where 4 x is conceded
// (tests/test_f64_split_gpu.py). f16 subnormal operands are honoured by the
// instruction (scripts/mfma_f16_ubench.hip), so small low parts are not lost: with N(0, 0.02)
// weights every low weight piece is subnormal, the kernel stays within 1.0 x that unit, and
// flushing them would cost over 100 x it (tests/test_split_f16_ref.py). |activations| must stay
// below the f16 range (65504); measured with pre-activations up to 1.2e4.
//
// Operand layout of the instruction: lane l supplies 8 consecutive k (8*(l>>5) .. +7) of row/column
// l&31; the result layout is the 32x32 f32 one. A result tile (16 registers per lane, features
// F(r,h) = (r&3) + 8(r>>2) + 4h) therefore splits into two k-sub-steps: registers 0..7 and 8..15.
//
// Everything is k-outer: a layer-1 output tile (32 features x 32 points) is produced — voxel part
// gathered as the accumulator's initial value, ray part as a rank-1 update, positional encoding
// as NK1 k-steps, IEF term as one more instruction — then activated, split and consumed by all
// layer-2 output tiles at once, so no tile of layer-1 or layer-2 outputs is ever held beyond its
// use and a wavefront needs < 256 registers: two workgroups per CU, whose matrix, vector and memory
// instructions overlap. The second IEF iteration recomputes layer 1 (+168 matrix instructions)
// instead of holding 128 registers across the pass.
//
// Weight stream ("H" layout): one section of 288 quads (1 KiB: 64 lanes x 8 halves) per decoder,
// in exactly the order PointsH::desc() gives; an IEF decoder's section is consumed once per
// iteration. It reaches the matrix instructions through the feed of lidf_split32.h, which also holds
// the section's tail, the steps of layers 2 to 4 and the packer that this kernel shares with
// lidf_rows_h.hip.
//
// Three instantiations of one body (PointsForm): the two-net launch over all pairs, one net of the
// two-net stream and tables over all pairs (offsets for the selected pairs only: prob_dec), and the
// list form of that (offset_dec on the one-pair-per-ray list, where every row is its own ray).
#include "lidf_launch.h"
#include "lidf_mma.h"
#include "lidf_split32.h"
#include <stdio.h>
#include <stdlib.h>

// development only: per-phase cycle counters of wavefront 0 of workgroup 0, written to a.out_base
#ifdef LIDF_PROFILE
#define PROF_DECL long long prof_t = clock64(); long long prof_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0}; const long long prof_w0 = wall_clock64(), prof_c0 = prof_t;
#define PROF(i) { long long t_ = clock64(); prof_acc[i] += t_ - prof_t; prof_t = t_; }
#define PROF_DUMP if (threadIdx.x == 0 && a.out_base) { long long* o_ = (long long*)a.out_base + 16 + 4 * blockIdx.x; o_[0] = prof_w0; o_[1] = wall_clock64(); o_[2] = __builtin_amdgcn_s_getreg(63492); o_[3] = __builtin_amdgcn_s_getreg(63508); } \
    if (blockIdx.x == 0 && threadIdx.x == 0 && a.out_base) { prof_acc[6] = wall_clock64() - prof_w0; prof_acc[7] = clock64() - prof_c0; for (int i_ = 0; i_ < 8; ++i_) ((long long*)a.out_base)[i_] = prof_acc[i_]; }
#else
#define PROF_DECL
#define PROF(i)
#define PROF_DUMP
#endif


#ifndef RING_D
#define RING_D 4  // quads of the stream in flight between LDS and the matrix instructions
#endif
#define NK1 LIDF_H_NK1            // layer-1 k-steps of 16: 6 of sin/cos (8 octaves) + raw x,y,z
#define PASS_QUADS LIDF_HPASS_QUADS
#define LDS_STREAM_ELEMS (NBUF * CH_ELEMS)
// + the tile-grab slot + 7 floats per lane of per-tile geometry parked outside the register file
// (28 B/lane: with it two workgroups use 163,632 of the CU's 163,840 B)
#define LDS_STASH_FLOATS 7
#define LDS_BYTES ((LDS_STREAM_ELEMS + 4 * NK1 * 64 + 1) * 16 + 4 * LDS_STASH_FLOATS * 64 * 4)
#define LIDF_H_GRAB 2

// ------------------------------------------------------------------------------------------------
// The kernel's policy (lidf_split32.h): its feed, the order of a decoder's section, its layer-1 quads
// ------------------------------------------------------------------------------------------------
struct PointsH {
    static constexpr int PASS = PASS_QUADS, RING = RING_D;
    // The staged chunk is published at position 4 and the barrier stands at position 6, behind lgkmcnt(2): the ring
    // reads of positions 5 and 6 were issued after the four writes, so the writes have landed once at most two
    // operations are outstanding, and the ring need not drain.
    static constexpr int PUBLISH_Q = 4, BARRIER_Q = 6, BARRIER_LGKM = 2;
    static constexpr bool L1_PREFIX = false, TILE_COUNTER = true;
    static constexpr int L1U = 2 * NK1 + 2;   // quads of one layer-1 tile: NK1 (hi, lo) pairs and the two mixed steps

    __host__ __device__ static constexpr QD l1u_desc(int T, int r) {
        if (r < 2 * NK1) return {K_L1, 0, T, r >> 1, r & 1, r >> 1};
        return {r == 2 * NK1 ? K_XA : K_XB, 0, T, 0, 0, 0};
    }
    __host__ __device__ static constexpr QD desc(int s) {
        if (s < 4) return {K_B2, s, 0, 0, 0, 0};
        s -= 4;
        if (s < L1U) return l1u_desc(0, s);
        s -= L1U;
        if (s < 7 * (L1U + 16)) {
            const int T = s / (L1U + 16), r = s % (L1U + 16);
            if (r < L1U) return l1u_desc(T + 1, r);  // layer 1 runs one tile ahead of layer 2
            return l2_desc(T, r - L1U);
        }
        return tail_desc(s - 7 * (L1U + 16));
    }

    __device__ static _Float16 l1_value(const NetW& n, const L1Map& m, const QD d, const int half, const int o,
                                        const int i) {
        const int col0 = half ? m.leave_c0 : m.enter_c0;   // lanes 0..31 weight the enter position, 32..63 the leave position
        const float* w = n.w1 + (size_t)(32 * d.T + o) * n.ld1;
        if (d.kind == K_L1) {
            // k-step ks: 4 (octave, coordinate) combos 4ks..4ks+3, element 2c' = sin, 2c'+1 = cos
            const int c = 4 * d.sub + (i >> 1), oct = c / 3, dd = c % 3;
            if (oct >= m.L) return (_Float16)0.f;
            return hpiece(w[col0 + 3 + 6 * oct + 3 * (i & 1) + dd], d.lo);
        }
        if (d.kind == K_XA)   // raw x, y, z: high weight pieces twice, against (xh, yh, zh, xl, yl, zl, 0, 0)
            return i < 6 ? hpiece(w[col0 + i % 3], 0) : (_Float16)0.f;
        // K_XB: (wlx, wly, wlz, uh, ray_hi, ray_lo, uh, ul) against (xh, yh, zh, vh, m, m, vl, vh): low weight pieces
        // of x, y, z; the IEF term u*val (lanes 0..31 only); elements 4, 5 are filled in by the kernel with the
        // raypart row of this half's ray
        if (i < 3) return hpiece(w[col0 + i], 1);
        if (i == 4 || i == 5 || half != 0 || !n.is_ief) return (_Float16)0.f;
        return hpiece(ief_u(n, 32 * d.T + o), i == 7 ? 1 : 0);
    }
};
static_assert(section_fits<PointsH>(4 + 8 * PointsH::L1U + 7 * 16), "section size");

extern "C" hipError_t lidf_launch_pack_h(const StreamLayout& lay, const NetW& n0, const NetW& n1,
                                         const L1Map& m, float* stream, float* aux,
                                         hipStream_t st) {
    return launch_pack_h<PointsH>(lay, n0, n1, m, stream, aux, st);
}

// FORM_ALL: both nets of the stream, tables of nets * 256 floats per row (the default launch).
// FORM_PART: the launch's nets are columns part_off.. of tables with part_ld floats per row (one net of
//            the two-net tables; the host points stream / aux at that net's section).
// FORM_LIST: FORM_PART on a one-pair-per-ray list. A 32-point tile has 32 rays there, which the rank-1
//            ray rounds would cover two at a time (16 instructions per layer-1 tile and pass), so the
//            ray row is gathered per lane like the voxel row: layer 1 starts from the f32 sum
//            voxpart[vid] + raypart[ray], no ray round runs, and a row's result depends on that row alone.
enum PointsForm { FORM_ALL = 0, FORM_PART = 1, FORM_LIST = 2 };

// What one pass needs to know about the points of this wavefront.
struct TileCtx {
    const float* vp;     // voxpart row of this lane's point (+ net, + 4*half)
    const float* rp;     // raypart row of this half's ray of round 0 (+ net, + lane&31);
                         // list form: of this lane's own ray (+ net, + 4*half)
    float rayB;          // packed (1,1) if this lane's point belongs to this half's ray
    int ray;             // this lane's ray (for the extra rounds)
    unsigned todo;       // points not covered by round 0 (0 in the common case)
    const float* rbase;  // raypart + net*256 + lane&31 (extra rounds)
    int ray_stride;      // nets*256
    int pl;              // LDS element index of this lane's low pieces of the embedding operands
};

// One decoder pass on the 32 points of this wavefront:
//   H1 = lrelu(W1 x + b1 [+ u*val]);  H2 = lrelu(W2 H1 + b2);  H3 = lrelu(W3 H2 + b3);  y = w4.H3 + b4
// with W1 x = voxpart[voxel] + raypart[ray] + W1[:, enter|leave] PE(position).
#ifdef LIDF_PROFILE_CHUNKS
__device__ long long g_chunk_ticks[32];
#define CHUNK_PROF(q, s_) if ((q) == CH_QUADS - 1) { const long long t_ = clock64(); if (blockIdx.x == 0 && threadIdx.x == 0) g_chunk_ticks[(s_) / CH_QUADS] += t_ - chunk_t; chunk_t = t_; }
#else
#define CHUNK_PROF(q, s_)
#endif
template <int FORM>
__device__ __forceinline__ float decoder_pass_h(Feed<PointsH>& f, const FeedCfg& c, f32x4* sb,
                                                const TileCtx& tc, const f32x4 (&pbh)[NK1],
                                                const f32x4 xaB, const float xyB, const _Float16 zh,
                                                const float val, const int h, const int col,
                                                const float* __restrict__ ax) {
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    const _Float16 one = (_Float16)1.f;
    const f32x4 onesB = ones_operand(h);
    f32x4 xbB = zero4;
    xbB[0] = xyB;
    {
        // (xh, yh, zh, vh, m, m, vl, vh): raw position, IEF input value, ray membership
        const _Float16 vh = (_Float16)val;
        const _Float16 vl = (_Float16)(val - (float)vh);
        xbB[1] = pack2(zh, vh);
        xbB[2] = tc.rayB;
        xbB[3] = pack2(vl, vh);
    }

    f32x16 a1[2];               // layer-1 tiles, ping-pong: accumulating / being split
    float rpv[2];               // raypart value of this lane's row, same ping-pong
    f32x4 bh[2], bl[2];         // split H1 tile, [k-sub-step] (single buffer, see below)
    f32x4 pl_cur = zero4, pl_nxt = zero4;  // low pieces of the embedding operand, from LDS
    TAIL32_STATE;               // layers 2 to 4

    // voxel part of tile T straight into the accumulator layout; ray part of this lane's row
    auto gather = [&](const int T) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const f32x4 v = *(const f32x4*)(tc.vp + T * 32 + 8 * g);
#pragma unroll
            for (int i = 0; i < 4; ++i) a1[T & 1][4 * g + i] = v[i];
        }
        if (FORM != FORM_LIST) rpv[T & 1] = tc.rp[T * 32];
    };
    // list form: the lane's own ray row, loaded with the voxel row and added to it (one f32 sum per
    // feature) before the tile's first matrix instruction; the loads have a layer-2 segment to land
    f32x4 rr[4];
    auto gather_ray = [&](const int T) {
#pragma unroll
        for (int g = 0; g < 4; ++g) rr[g] = *(const f32x4*)(tc.rp + T * 32 + 8 * g);
    };
    auto add_ray = [&](const int T) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
#pragma unroll
            for (int i = 0; i < 4; ++i) a1[T & 1][4 * g + i] = __fadd_rn(a1[T & 1][4 * g + i], rr[g][i]);
        }
    };
    gather(0);
    if (FORM == FORM_LIST) {
        gather_ray(0);
        add_ray(0);
    }
    gather(1);
    if (FORM == FORM_LIST) {
        gather_ray(1);
        add_ray(1);
    }
    pl_cur = sb[tc.pl];
#ifdef LIDF_PROFILE_CHUNKS
    long long chunk_t = clock64();
#endif

#pragma unroll
    for (int s = 0; s < PASS_QUADS; ++s) {
        const int Q = s % CH_QUADS;
        const QD d = PointsH::desc(s);
        const f32x4 A = feed_take(f, c, sb, Q);
        if (d.kind == K_L1) {
            f32x16& acc = a1[d.T & 1];
            if (!d.lo) {
                acc = MFMAH(A, pbh[d.sub], acc);
                acc = MFMAH(A, pl_cur, acc);
                // low pieces of the next k-step's operand (wraps to k-step 0 for the next tile)
                pl_nxt = sb[tc.pl + ((d.sub + 1) % NK1) * 64];
                // split the previous tile behind these matrix instructions (8 pairs over the
                // NK1 k-steps and the two mixed steps that follow)
                if (d.T >= 1) prep_pairs(d.sub, d.sub + 1, a1[(d.T - 1) & 1], bh, bl);
            } else {
                acc = MFMAH(A, pbh[d.sub], acc);
                pl_cur = pl_nxt;
            }
        } else if (d.kind == K_XA) {
            a1[d.T & 1] = MFMAH(A, xaB, a1[d.T & 1]);
            if (d.T >= 1) prep_pairs(NK1, NK1 + 1, a1[(d.T - 1) & 1], bh, bl);
        } else if (d.kind == K_XB) {
            // elements 4, 5 of the weights fragment <- (hi, lo) of the raypart row of this half's
            // ray: the ray part of layer 1 is a rank-1 update, two rays per instruction. Tiles that
            // straddle more than two rays (ragged scenes) take extra rounds.
            f32x16& acc = a1[d.T & 1];
            // (list form: the ray row is in the accumulator already; elements 4, 5 stay the packer's
            // zeros against rayB = 0)
            f32x4 Ar = A;
            if (FORM != FORM_LIST) Ar[2] = split1(rpv[d.T & 1]);
            acc = MFMAH(Ar, xbB, acc);
            if (d.T >= 1) prep_pairs(NK1 + 1, 8, a1[(d.T - 1) & 1], bh, bl);
            if (FORM != FORM_LIST && tc.todo) {
                unsigned todo = tc.todo;
                while (todo) {
                    const int p0 = __builtin_ctz(todo);
                    const int r0 = __builtin_amdgcn_readlane(tc.ray, p0);
                    const unsigned m0 = (unsigned)__ballot(tc.ray == r0) & todo;
                    todo &= ~m0;
                    int r1 = r0;
                    unsigned m1 = 0;
                    if (todo) {
                        const int p1 = __builtin_ctz(todo);
                        r1 = __builtin_amdgcn_readlane(tc.ray, p1);
                        m1 = (unsigned)__ballot(tc.ray == r1) & todo;
                        todo &= ~m1;
                    }
                    const float v = tc.rbase[(size_t)(h ? r1 : r0) * tc.ray_stride + d.T * 32];
                    f32x4 xa = zero4, xb = zero4;
                    xa[2] = split1(v);
                    xb[2] = (((h ? m1 : m0) >> col) & 1u) ? pack2(one, one) : 0.f;
                    acc = MFMAH(xa, xb, acc);
                }
            }
        } else {
            if (d.kind == K_L2 && !d.lo) {
                // the tile after next can start loading: its accumulator is free once the split
                // of tile T (same parity) is done
                if (d.j == 0 && d.T + 2 < 8) {
                    gather(d.T + 2);
                    if (FORM == FORM_LIST) gather_ray(d.T + 2);
                }
                if (FORM == FORM_LIST && d.j == 7 && d.T + 2 < 8) add_ray(d.T + 2);
                // tile 7 has no layer-1 segment after it to hide its split behind, and a second
                // operand buffer just for it would push the kernel into spilling
                if (d.T == 7 && d.j == 0) prep_pairs(0, 8, a1[1], bh, bl);
            }
            // operands of layer 4, fetched late and in two halves so that they do not hold 32 registers
            // through layer 3; their latency still hides behind it
            if (d.kind == K_L3 && !d.lo && d.j == 0 && d.T >= 2) tail_load_w4(w4, ax, h, 4 * (d.T - 2), 4 * (d.T - 1));
            tail_step(TAIL32_ARGS, d, A, onesB, bh, bl);
            if (d.kind == K_B3 && d.t == 0) b4 = ax[64];
        }
        CHUNK_PROF(Q, s)
        SCHED_FENCE();
    }
#ifdef LIDF_PROFILE_CHUNKS
    if (blockIdx.x == 0 && threadIdx.x == 0) { g_chunk_ticks[31] += 1; }
#endif
    return tail_finish(TAIL32_ARGS, b4);
}

struct GeoH {
    int ray, vid;
    float te, tl, dx, dy, dz;
};

template <int FORM>
__global__ void __launch_bounds__(256, 2) lidf_points_h_kernel(PointsArgs a) {
    extern __shared__ f32x4 sb[];  // [NBUF chunks of the stream][per wavefront: NK1 operand quads]
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int h = lane >> 5;
    const int col = lane & 31;

    const FeedCfg c = feed_cfg(a, lane, wave);

    // 128-point tiles are handed out dynamically, LIDF_H_GRAB at a time, from a counter the packer
    // zeroes: the two workgroups of a CU do not progress at the same rate (the older one wins the
    // issue arbitration), and with a static split the younger one would run the tail alone.
    // Every wavefront of the workgroup runs the same tiles (the stream is shared); out-of-range
    // points are clamped.
    const long long AN = a.n_dev ? (long long)*a.n_dev : a.n;   // device-side count (the frame path)
    const long long ntile = (AN + 127) / 128;
    int* const grab_slot = (int*)(sb + LDS_STREAM_ELEMS + 4 * NK1 * 64);
    // geometry that is only needed again at the end of the tile (the offset net's output, the next
    // tile's indices) waits in LDS instead of occupying registers through every pass
    float* const stash = (float*)(sb + LDS_STREAM_ELEMS + 4 * NK1 * 64 + 1) +
                         wave * (LDS_STASH_FLOATS * 64) + lane;

    Feed<PointsH> f;
    feed_start(f, c, sb);

    // addresses = wave-uniform base (SGPRs) + a 32-bit lane offset: no 64-bit pointer registers
    auto load_idx = [&](long long tile, GeoH& g) {
        const long long last = AN - 1;
        long long t0 = tile * 128;                  // uniform
        if (t0 > last) t0 = last & ~127LL;          // a prefetch past the end re-reads the last tile
        const long long rem = last - t0;
        const int lo = wave * 32 + col;
        const unsigned off = (unsigned)(lo < rem ? lo : rem);  // out-of-range points are clamped
        g.ray = (a.pair_ray + t0)[off];
        g.vid = (a.pair_vox + t0)[off];
        const f32x2 tt = *(const f32x2*)((const char*)(a.pair_t + 2 * t0) + 8u * off);
        g.te = tt[0];
        g.tl = tt[1];
    };
    auto load_dir = [&](GeoH& g) {
        const char* rd = (const char*)a.ray_dir + 12u * (unsigned)g.ray;
        g.dx = *(const float*)(rd + 0);
        g.dy = *(const float*)(rd + 4);
        g.dz = *(const float*)(rd + 8);
    };
    GeoH cur = {}, nxt = {}, nx2 = {};

    // floats per row of the two tables / first column of this launch's nets
    const int part_ld = FORM == FORM_ALL ? a.nets * 256 : a.part_ld;
    const int part_off = FORM == FORM_ALL ? 0 : a.part_off;
    TileCtx tc;
    tc.pl = LDS_STREAM_ELEMS + wave * NK1 * 64 + lane;
    tc.ray_stride = part_ld;

    PROF_DECL
    for (;;) {
    if (threadIdx.x == 0) *grab_slot = atomicAdd(a.tile_counter, LIDF_H_GRAB);
    __syncthreads();
    const long long tb = __builtin_amdgcn_readfirstlane(*grab_slot);
    if (tb >= ntile) break;
    const long long te_ = tb + LIDF_H_GRAB < ntile ? tb + LIDF_H_GRAB : ntile;
    load_idx(tb, cur);
    if (FORM != FORM_LIST) load_idx(tb + 1, nxt);
    load_dir(cur);
    for (long long tile = tb; tile < te_; ++tile) {
        PROF(0)
        const long long p = tile * 128 + wave * 32 + col;
        const bool valid = p < AN;
        // (list form: no prefetch. The next tile's geometry is loaded after this tile's passes, at the foot of
        // the loop, so that nothing of it occupies registers through them; that load is exposed, once per
        // tile of n_iter passes)
        if (FORM != FORM_LIST) {
            load_dir(nxt);
            load_idx(tile + 2, nx2);
        }
        // this half's embedding input: lanes 0..31 embed the enter position, lanes 32..63 the leave
        // position (pipeline.py:349-360; 'rel' subtracts the voxel centre)
        const float tt = h ? cur.tl : cur.te;
        float px = __fmul_rn(cur.dx, tt);
        float py = __fmul_rn(cur.dy, tt);
        float pz = __fmul_rn(cur.dz, tt);
        if (a.pos_rel) {
            px -= a.vox_center[3 * (size_t)cur.vid + 0];
            py -= a.vox_center[3 * (size_t)cur.vid + 1];
            pz -= a.vox_center[3 * (size_t)cur.vid + 2];
        }
        stash[0 * 64] = cur.te;
        stash[1 * 64] = cur.dx;
        stash[2 * 64] = cur.dy;
        stash[3 * 64] = cur.dz;
        if (FORM != FORM_LIST) {
            stash[4 * 64] = nxt.te;
            stash[5 * 64] = nxt.tl;
            stash[6 * 64] = __int_as_float(nxt.vid);
        }
        // operands of the layer-1 k-steps, shared by all passes of this tile: high pieces in
        // registers, low pieces in this wavefront's LDS rows
        f32x4 pbh[NK1];
        {
            const Rev rv[3] = {to_rev(px), to_rev(py), to_rev(pz)};
#pragma unroll
            for (int ks = 0; ks < NK1; ++ks) {
                f32x4 lo4;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int idx = 4 * ks + i;  // combo: octave idx/3, coordinate idx%3
                    float sv, cv, hi, lo;
                    rev_sincos(rv[idx % 3], (float)(1 << (idx / 3)), sv, cv);
                    split2(sv, cv, hi, lo);
                    pbh[ks][i] = hi;
                    lo4[i] = lo;
                }
                sb[tc.pl + ks * 64] = lo4;
            }
        }
        // raw position against the two mixed k-steps: (xh, yh, zh, xl, yl, zl, 0, 0) and the
        // (xh, yh, zh, .) head of the second one. (zh travels as a scalar: extracting it from a
        // packed word made hipcc 7.2 pick the low half of the wrong register.)
        f32x4 xaB = {0.f, 0.f, 0.f, 0.f};
        float xyB;
        const _Float16 zh = (_Float16)pz;
        {
            const _Float16 xh = (_Float16)px, yh = (_Float16)py;
            const _Float16 xl = (_Float16)(px - (float)xh), yl = (_Float16)(py - (float)yh),
                           zl = (_Float16)(pz - (float)zh);
            xaB[0] = pack2(xh, yh);
            xaB[1] = pack2(zh, xl);
            xaB[2] = pack2(yl, zl);
            xyB = pack2(xh, yh);
        }
        // rays of this wavefront's 32 points: round 0 covers the first two distinct rays
        // (list form: every lane gathers the row of its own ray, there are no rounds)
        int my_ray = cur.ray;
        if (FORM == FORM_LIST) {
            tc.rayB = 0.f;
            tc.todo = 0;
            tc.ray = cur.ray;
        } else {
            unsigned todo = (unsigned)__ballot(h == 0);
            const int p0 = __builtin_ctz(todo);
            const int r0 = __builtin_amdgcn_readlane(cur.ray, p0);
            const unsigned m0 = (unsigned)__ballot(cur.ray == r0) & todo;
            todo &= ~m0;
            int r1 = r0;
            unsigned m1 = 0;
            if (todo) {
                const int p1 = __builtin_ctz(todo);
                r1 = __builtin_amdgcn_readlane(cur.ray, p1);
                m1 = (unsigned)__ballot(cur.ray == r1) & todo;
                todo &= ~m1;
            }
            my_ray = h ? r1 : r0;
            tc.rayB = (((h ? m1 : m0) >> col) & 1u) ? pack2((_Float16)1.f, (_Float16)1.f) : 0.f;
            tc.todo = todo;
            tc.ray = cur.ray;
        }
        PROF(1)

        for (int net = 0; net < a.nets; ++net) {
            if (FORM == FORM_ALL) {
                tc.vp = a.voxpart + ((size_t)cur.vid * a.nets + net) * 256 + 4 * h;
                tc.rp = a.raypart + ((size_t)my_ray * a.nets + net) * 256 + col;
                tc.rbase = a.raypart + net * 256 + col;
            } else {
                tc.vp = a.voxpart + (size_t)cur.vid * part_ld + part_off + net * 256 + 4 * h;
                tc.rp = a.raypart + (size_t)my_ray * part_ld + part_off + net * 256 +
                        (FORM == FORM_LIST ? 4 * h : col);
                tc.rbase = a.raypart + part_off + net * 256 + col;
            }
            float val = a.init[net];
            const float* ax = a.aux + net * LIDF_AUX_FLOATS;
            const int npass = a.npass[net];
            for (int pass = 0; pass < npass; ++pass)
                val += decoder_pass_h<FORM>(f, c, sb, tc, pbh, xaB, xyB, zh, val, h, col, ax);
            PROF(2 + net)

            // ---------------- outputs ----------------
            if (valid && h == 0) {
                const float o = out_act(val, a.sigmoid[net]);
                if (a.out[net]) a.out[net][p] = o;
                if (a.is_offset[net]) {
                    // pipeline.py:437-439, same operation order in f32
                    const float te = stash[0 * 64], dx = stash[1 * 64], dy = stash[2 * 64],
                                dz = stash[3 * 64];
                    const float ex = __fmul_rn(dx, te);
                    const float ey = __fmul_rn(dy, te);
                    const float ez = __fmul_rn(dz, te);
                    float s = __fadd_rn(__fmul_rn(o, a.rscale), a.r0);
                    s = __fmul_rn(__fmul_rn(s, a.sqrt3), a.part_size);
                    a.pair_pred_pos[3 * p + 0] = __fadd_rn(ex, __fmul_rn(s, dx));
                    a.pair_pred_pos[3 * p + 1] = __fadd_rn(ey, __fmul_rn(s, dy));
                    a.pair_pred_pos[3 * p + 2] = __fadd_rn(ez, __fmul_rn(s, dz));
                }
            }
        }
        if (FORM == FORM_LIST) {
            load_idx(tile + 1, cur);
            load_dir(cur);
            continue;
        }
        cur.ray = nxt.ray;
        cur.dx = nxt.dx;
        cur.dy = nxt.dy;
        cur.dz = nxt.dz;
        cur.te = stash[4 * 64];
        cur.tl = stash[5 * 64];
        cur.vid = __float_as_int(stash[6 * 64]);
        nxt.ray = nx2.ray;
        nxt.vid = nx2.vid;
        nxt.te = nx2.te;
        nxt.tl = nx2.tl;
    }
    }
    PROF_DUMP
}

// form: a PointsForm. FORM_ALL ignores part_ld / part_off (tables of nets * 256 floats per row); the other two
// need part_ld > 0. FORM_LIST: a.pair_* are a one-pair-per-ray list.
static hipError_t launch_points_h_form(const PointsArgs& a, int form, int cus, hipStream_t st) {
    if (a.n <= 0) return hipSuccess;
    if (form != FORM_ALL && a.part_ld <= 0) return hipErrorInvalidValue;
    const void* const kern = form == FORM_ALL    ? (const void*)lidf_points_h_kernel<FORM_ALL>
                             : form == FORM_PART ? (const void*)lidf_points_h_kernel<FORM_PART>
                                                 : (const void*)lidf_points_h_kernel<FORM_LIST>;
    // > 64 KiB of dynamic LDS needs the opt-in once per device and kernel (one process may drive several)
    static bool configured[3][64] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return hipErrorInvalidDevice;
    if (!configured[form][dev]) {
        hipError_t e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES);
        if (e != hipSuccess) return e;
        configured[form][dev] = true;
#ifdef LIDF_PROFILE
        for (int lds = 32768; lds <= LDS_BYTES + 8192; lds += 4096) {
            int nb = -1;
            hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kern, 256, lds);
            fprintf(stderr, "occupancy with %d B of LDS per workgroup: %d workgroups per CU\n", lds, nb);
        }
#endif
    }
    // two workgroups per CU
    const long long ntile = (a.n + 127) / 128;
    int grid = (int)(ntile < 2LL * cus ? ntile : 2LL * cus);
#ifdef LIDF_PROFILE
    if (getenv("LIDF_H_SOLO")) grid = cus;
#endif
#ifdef LIDF_PROFILE_CHUNKS
    static long long zero_[32] = {0};
    hipMemcpyToSymbolAsync(HIP_SYMBOL(g_chunk_ticks), zero_, sizeof(zero_), 0, hipMemcpyHostToDevice, st);
#endif
    if (form == FORM_ALL)
        hipLaunchKernelGGL(lidf_points_h_kernel<FORM_ALL>, dim3(grid), dim3(256), LDS_BYTES, st, a);
    else if (form == FORM_PART)
        hipLaunchKernelGGL(lidf_points_h_kernel<FORM_PART>, dim3(grid), dim3(256), LDS_BYTES, st, a);
    else
        hipLaunchKernelGGL(lidf_points_h_kernel<FORM_LIST>, dim3(grid), dim3(256), LDS_BYTES, st, a);
#ifdef LIDF_PROFILE_CHUNKS
    {
        long long t_[32];
        hipMemcpyFromSymbol(t_, HIP_SYMBOL(g_chunk_ticks), sizeof(t_), 0, hipMemcpyDeviceToHost);
        fprintf(stderr, "passes of workgroup 0: %lld ; ticks per chunk (avg per pass):", t_[31]);
        for (int i = 0; i < PASS_QUADS / CH_QUADS; ++i) fprintf(stderr, " %lld", t_[31] ? t_[i] / t_[31] : 0);
        fprintf(stderr, "\n");
    }
#endif
    return hipGetLastError();
}

// all pairs: both nets (part_ld == 0) or the launch's nets inside wider tables (part_ld > 0)
extern "C" hipError_t lidf_launch_points_h(const PointsArgs& a, int cus, hipStream_t st) {
    return launch_points_h_form(a, a.part_ld > 0 ? FORM_PART : FORM_ALL, cus, st);
}

// a one-pair-per-ray list (offsets for the selected pairs only)
extern "C" hipError_t lidf_launch_points_h_list(const PointsArgs& a, int cus, hipStream_t st) {
#ifdef LIDF_H_LIST_ROUNDS   // development only (A/B): the list through the rank-1 ray rounds
    return launch_points_h_form(a, FORM_PART, cus, st);
#else
    return launch_points_h_form(a, FORM_LIST, cus, st);
#endif
}
