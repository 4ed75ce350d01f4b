// lidf_split32.h — what the two split-f16 decoders on 32 x 32 tiles share (precision = "f16x3"; gfx950 only), one
// definition each: lidf_points_h.hip (the fused per-point query) and lidf_rows_h.hip (the decoder on materialised rows)
// keep their layer-1 formulation, their kernel bodies around the pass and their launchers.
//
//   Feed        the weight stream's way from global memory to the matrix instructions. The four wavefronts of a
//               workgroup consume the stream in lockstep; it is staged once per workgroup through LDS in chunks of
//               CH_QUADS quads (NBUF rotating buffers, one s_barrier per chunk, global loads issued one chunk ahead),
//               and each wavefront keeps a register ring of ds_read_b128 in flight.
//   tail_desc   the order of a decoder's section from the last layer-2 segment on.
//   tail_step   layers 2 to 4 of one pass: the matrix and prep_pairs schedule of the steps both kernels take.
//   the packer  one thread per f16 element of the stream; the layer-1 quads come from the kernel's policy.
//
// A kernel describes itself by a policy struct P:
//   PASS          quads of a decoder's pass section (whole chunks)
//   RING          quads in flight between LDS and the matrix instructions
//   PUBLISH_Q     position of a chunk at which the staged chunk after the next goes to LDS and the next global fetch
//                 starts
//   BARRIER_Q, BARRIER_LGKM   position of the chunk's barrier and the LDS operations that may be outstanding at it
//   L1_PREFIX     a net's section opens with lay.l1_quads of layer 1 (FeedCfg::nk1 chunks), streamed once per net
//                 in front of its passes
//   TILE_COUNTER  the packer zeroes the kernel's tile hand-out counter behind the aux array
//   desc(s)       the QD of quad s of the pass section
//   l1_prefix_value(n, m, quad, half, o, i), l1_value(n, m, d, half, o, i)   the packer's layer-1 elements: of the
//                 prefix, and of the kinds of desc() that are not listed under "shared" below
#pragma once
#include "lidf_launch.h"
#include "lidf_mma.h"

// ------------------------------------------------------------------------------------------------
// Order of a decoder's pass section (shared by the packer and the kernels)
// ------------------------------------------------------------------------------------------------
enum {
    K_B2 = 0, K_L2, K_B3, K_L3, K_PAD,   // shared
    K_L1, K_XA, K_XB,                    // lidf_points_h.hip: layer 1 is interleaved with layer 2
    K_U,                                 // lidf_rows_h.hip: the IEF term on the held layer-1 result
};
struct QD {
    int kind;
    int t;    // output tile
    int T;    // layer 1 / u: the H1 tile produced; layers 2, 3: the input tile consumed
    int sub;  // layer 1: k-step; layers 2, 3: k-sub-step inside the input tile
    int lo;   // 0: high pieces of the weights, 1: low pieces
    int j;    // ordinal of the (hi, lo) pair inside its segment
};
// segment T < 7 of layer 2, quad r of 16: k-sub-step major, all four output tiles advance together
__host__ __device__ constexpr QD l2_desc(int T, int r) {
    const int lo = r & 1, j = r >> 1;
    return {K_L2, j & 3, T, j >> 2, lo, j};
}
// From the last layer-2 segment on (s counted from its first quad): that segment tile-major, so that the output tiles
// finish one by one and their split hides behind the rest; b3; layer 3 with its last segment tile-major; padding.
#define TAIL_QUADS (16 + 2 + 32)
__host__ __device__ constexpr QD tail_desc(int s) {
    if (s < 16) {
        const int lo = s & 1, j = s >> 1;
        return {K_L2, j >> 1, 7, j & 1, lo, j};
    }
    s -= 16;
    if (s < 2) return {K_B3, s, 0, 0, 0, 0};
    s -= 2;
    if (s < 32) {
        const int T = s / 8, r = s % 8, lo = r & 1, j = r >> 1;
        if (T < 3) return {K_L3, j & 1, T, j >> 1, lo, j};
        return {K_L3, j >> 1, T, j & 1, lo, j};
    }
    return {K_PAD, 0, 0, 0, 0, 0};
}
// head_quads: what the kernel's own desc() puts in front of the tail
template <class P>
constexpr bool section_fits(int head_quads) {
    return head_quads + TAIL_QUADS <= P::PASS && P::PASS % CH_QUADS == 0;
}

// ------------------------------------------------------------------------------------------------
// Packer: one thread per f16 element.
// ------------------------------------------------------------------------------------------------
template <class P>
__device__ _Float16 stream_value_h(const StreamLayout& lay, const NetW& net0, const NetW& net1, const L1Map& m,
                                   long long e) {
    const int per_net = lay.net_quads * 512;
    const int net = (int)(e / per_net);
    e %= per_net;
    const NetW& n = net ? net1 : net0;
    int quad = (int)(e / 512);
    const int lane = (int)(e % 512) / 8, i = (int)(e & 7);
    const int half = lane >> 5, o = lane & 31;
    if constexpr (P::L1_PREFIX) {
        if (quad < lay.l1_quads) return P::l1_prefix_value(n, m, quad, half, o, i);
        quad -= lay.l1_quads;
    }
    const QD d = P::desc(quad);
    switch (d.kind) {
        case K_B2:
            return half == 0 && i < 3 ? hpiece(n.b2[32 * d.t + o], i) : (_Float16)0.f;
        case K_B3:
            return half == 0 && i < 3 ? hpiece(n.b3[32 * d.t + o], i) : (_Float16)0.f;
        case K_L2:
            return hpiece(n.w2[(size_t)(32 * d.t + o) * LIDF_H1 + 32 * d.T +
                               tile_feature(8 * d.sub + i, half)], d.lo);
        case K_L3:
            return hpiece(n.w3[(size_t)(32 * d.t + o) * LIDF_H2 + 32 * d.T +
                               tile_feature(8 * d.sub + i, half)], d.lo);
        case K_PAD:
            return (_Float16)0.f;
        default:
            return P::l1_value(n, m, d, half, o, i);
    }
}

template <class P>
__global__ void lidf_pack_h_kernel(StreamLayout lay, NetW net0, NetW net1, L1Map m, _Float16* stream,
                                   float* aux) {
    if (lay.guard && lay.guard->dirty == 0) return;   // guarded packing: fingerprint unchanged
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < (long long)lay.total * 2) stream[e] = stream_value_h<P>(lay, net0, net1, m, e);
    if (aux && e < lay.nets * LIDF_AUX_FLOATS) pack_aux_h(net0, net1, e, aux);
    if (P::TILE_COUNTER && e == 0) ((int*)aux)[lay.nets * LIDF_AUX_FLOATS] = 0;
}

template <class P>
static hipError_t launch_pack_h(const StreamLayout& lay, const NetW& n0, const NetW& n1, const L1Map& m,
                                float* stream, float* aux, hipStream_t st) {
    const long long total = (long long)lay.total * 2;
    const int blocks = (int)((total + 255) / 256);
    hipLaunchKernelGGL(lidf_pack_h_kernel<P>, dim3(blocks), dim3(256), 0, st, lay, n0, n1, m, (_Float16*)stream,
                       aux);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// The stream feed of one wavefront.
// ------------------------------------------------------------------------------------------------
template <class P>
struct Feed {
    // Ring slots are static: position Q of a chunk uses slot Q % RING. The first ring read of the next buffer comes
    // at position CH_QUADS - RING, after the barrier. LDS operations complete in order, so at the barrier the
    // publishing writes have landed once no more operations are outstanding than were issued after them — one ring
    // read per position.
    static_assert(P::PASS % CH_QUADS == 0 && CH_QUADS % P::RING == 0, "sections are whole chunks of whole rings");
    static_assert(P::PUBLISH_Q <= P::BARRIER_Q && P::BARRIER_Q < CH_QUADS - P::RING &&
                      P::BARRIER_LGKM <= P::BARRIER_Q - P::PUBLISH_Q,
                  "publish, then barrier, then the ring's first read of the next chunk");
    f32x4 ring[P::RING];  // next RING quads
    f32x4 stage[4];  // this wavefront's quarter of the chunk after the next one, in flight
    int cur, nxt;    // element index (f32x4 units) of this lane in the current / next LDS buffer
    int nb;          // index of the next buffer
    int s_net, s_pass, s_idx;  // sequencer: which chunk the next global load fetches (s_pass -1: the layer-1 prefix)
};

struct FeedCfg {
    __amdgpu_buffer_rsrc_t srs;
    int vq;         // lane * 16
    int wave, lane;
    int net_bytes, nets;
    int nk1;        // chunks of the layer-1 prefix (read by L1_PREFIX policies only)
    int npass0, npass1;
};

__device__ __forceinline__ FeedCfg feed_cfg(const PointsArgs& a, const int lane, const int wave) {
    FeedCfg c;
    c.srs = __builtin_amdgcn_make_buffer_rsrc((void*)a.stream, 0, a.nets * a.net_quads * 1024, 0x00020000);
    c.vq = lane * 16;
    c.wave = wave;
    c.lane = lane;
    c.net_bytes = a.net_quads * 1024;
    c.nk1 = a.l1_quads / CH_QUADS;
    c.nets = a.nets;
    c.npass0 = a.npass[0];
    c.npass1 = a.npass[1];
    return c;
}

template <class P>
__device__ __forceinline__ void feed_issue(Feed<P>& f, const FeedCfg& c) {
    const bool prefix = P::L1_PREFIX && f.s_pass < 0;
    const int chunk = P::L1_PREFIX && !prefix ? c.nk1 + f.s_idx : f.s_idx;
    const int off = f.s_net * c.net_bytes + chunk * (CH_QUADS * 1024) + c.wave * 4096;
#pragma unroll
    for (int j = 0; j < 4; ++j) f.stage[j] = LDQ(c.srs, c.vq + j * 1024, off);
    // advance the sequencer: a decoder's pass section is consumed once per pass, its prefix once
    const int lim = prefix ? c.nk1 : P::PASS / CH_QUADS;
    if (++f.s_idx == lim) {
        f.s_idx = 0;
        const int np = f.s_net ? c.npass1 : c.npass0;
        if (++f.s_pass == np) {
            f.s_pass = P::L1_PREFIX ? -1 : 0;
            if (++f.s_net == c.nets) f.s_net = 0;
        }
    }
}

// prologue: chunk 0 into buffer 0, chunk 1 in flight, the ring filled
template <class P>
__device__ __forceinline__ void feed_start(Feed<P>& f, const FeedCfg& c, f32x4* sb) {
    f.s_net = 0;
    f.s_pass = P::L1_PREFIX ? -1 : 0;
    f.s_idx = 0;
    feed_issue(f, c);
#pragma unroll
    for (int j = 0; j < 4; ++j) sb[(4 * c.wave + j) * 64 + c.lane] = f.stage[j];
    feed_issue(f, c);
    __syncthreads();
    f.cur = c.lane;
    f.nb = 1;
    f.nxt = CH_ELEMS + c.lane;
#pragma unroll
    for (int i = 0; i < P::RING; ++i) f.ring[i] = sb[f.cur + i * 64];
}

// position Q (0..15) of the current chunk: returns the quad, refills the ring RING quads ahead, publishes the staged
// chunk to LDS and starts the next global fetch at PUBLISH_Q, and meets the other wavefronts at BARRIER_Q
template <class P>
__device__ __forceinline__ f32x4 feed_take(Feed<P>& f, const FeedCfg& c, f32x4* sb, const int Q) {
    const int slot = Q % P::RING;
    const f32x4 a = f.ring[slot];
    if (Q + P::RING < CH_QUADS)
        f.ring[slot] = sb[f.cur + (Q + P::RING) * 64];
    else
        f.ring[slot] = sb[f.nxt + (Q + P::RING - CH_QUADS) * 64];
    if (Q == P::PUBLISH_Q) {
        // The buffer written here last held the chunk before the previous one: every wavefront
        // finished reading it before it passed the previous barrier.
#pragma unroll
        for (int j = 0; j < 4; ++j) sb[f.nb * CH_ELEMS + (4 * c.wave + j) * 64 + c.lane] = f.stage[j];
        feed_issue(f, c);
    }
    if (Q == P::BARRIER_Q) asm volatile("s_waitcnt lgkmcnt(%0)\n\ts_barrier" ::"n"(P::BARRIER_LGKM) : "memory");
    if (Q == CH_QUADS - 1) {
        f.cur = f.nxt;
        f.nb = f.nb == NBUF - 1 ? 0 : f.nb + 1;
        f.nxt = f.nb * CH_ELEMS + c.lane;
    }
    return a;
}

// ------------------------------------------------------------------------------------------------
// Layers 2 to 4 of one decoder pass on the 32 points of a wavefront:
//   H2 = lrelu(W2 H1 + b2);  H3 = lrelu(W3 H2 + b3);  y = w4.H3 + b4
// ------------------------------------------------------------------------------------------------
// The caller owns the state: each piece is an array of its own, not a member of one struct. As one struct the fused
// kernel's list form went from 252 registers to 256 and 20 bytes of scratch per lane.
#define TAIL32_STATE                                                                                          \
    f32x16 acc2[4], acc3[2];   /* layer-2 and layer-3 output tiles */                                         \
    f32x4 gh[4][2], gl[4][2];  /* split H2 tiles, [tile][k-sub-step] */                                       \
    f32x4 w4[8];               /* layer 4 by (half, register) of the two layer-3 tiles; the caller fetches */ \
    float b4 = 0.f;            /* it (tail_load_w4) and b4 = aux[64] where its registers allow */             \
    float ys[4] = {0.f, 0.f, 0.f, 0.f}
#define TAIL32_PARAMS \
    f32x16(&acc2)[4], f32x16(&acc3)[2], f32x4(&gh)[4][2], f32x4(&gl)[4][2], f32x4(&w4)[8], float(&ys)[4]
#define TAIL32_ARGS acc2, acc3, gh, gl, w4, ys

// the operand that adds a bias quad's three pieces: (1, 1, 1, 0, ...) in the first half-wave
__device__ __forceinline__ f32x4 ones_operand(const int h) {
    f32x4 onesB = {0.f, 0.f, 0.f, 0.f};
    if (!h) {
        onesB[0] = pack2((_Float16)1.f, (_Float16)1.f);
        onesB[1] = pack2((_Float16)1.f, (_Float16)0.f);
    }
    return onesB;
}

__device__ __forceinline__ void tail_load_w4(f32x4 (&w4)[8], const float* __restrict__ ax, const int h, const int i0,
                                             const int i1) {
#pragma unroll
    for (int i = i0; i < i1; ++i) w4[i] = *(const f32x4*)(ax + h * 32 + 4 * i);
}

// Quad A of step d (kinds K_B2, K_L2, K_B3, K_L3; d is a compile-time constant after unrolling). bh / bl: the split
// H1 tile that layer 2 consumes at this step, [k-sub-step]. Splitting H1 behind the layer-2 segments T < 7 is the
// caller's.
__device__ __forceinline__ void tail_step(TAIL32_PARAMS, const QD d, const f32x4 A, const f32x4 onesB,
                                          const f32x4 (&bh)[2], const f32x4 (&bl)[2]) {
    const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (d.kind == K_B2) {
        acc2[d.t] = MFMAH(A, onesB, zero16);
    } else if (d.kind == K_L2) {
        acc2[d.t] = MFMAH(A, bh[d.sub], acc2[d.t]);
        if (!d.lo) {
            acc2[d.t] = MFMAH(A, bl[d.sub], acc2[d.t]);
            if (d.T == 7) {
                // last segment (tile-major): output tiles complete one by one
                if (d.j >= 2 && d.j < 6) prep_pairs(2 * (d.j - 2), 2 * (d.j - 2) + 2, acc2[0], gh[0], gl[0]);
                if (d.j >= 6) prep_pairs(2 * (d.j - 6), 2 * (d.j - 6) + 2, acc2[1], gh[1], gl[1]);
            }
        }
    } else if (d.kind == K_B3) {
        acc3[d.t] = MFMAH(A, onesB, zero16);
    } else if (d.kind == K_L3) {
        acc3[d.t] = MFMAH(A, gh[d.T][d.sub], acc3[d.t]);
        if (!d.lo) {
            acc3[d.t] = MFMAH(A, gl[d.T][d.sub], acc3[d.t]);
            // pending splits: segment T handles the second half of H2[T+1] (first two pairs)
            // and the first half of H2[T+2] (last two pairs)
            if (d.T < 3 && d.j < 2) prep_pairs(4 + 2 * d.j, 6 + 2 * d.j, acc2[d.T + 1], gh[d.T + 1], gl[d.T + 1]);
            if (d.T < 2 && d.j >= 2) prep_pairs(2 * (d.j - 2), 2 * (d.j - 2) + 2, acc2[d.T + 2], gh[d.T + 2], gl[d.T + 2]);
            if (d.T == 3 && d.j >= 2) {
                // acc3[0] is complete: its half of layer 4 runs behind acc3[1]'s last steps
#pragma unroll
                for (int r = 8 * (d.j - 2); r < 8 * (d.j - 2) + 8; ++r)
                    ys[r & 3] = fmaf(w4[r >> 2][r & 3], lrelu1(acc3[0][r]), ys[r & 3]);
            }
        }
    }
}

// layer 4 (64 -> 1) on the VALU, second tile; halves combined with one cross-half shuffle
__device__ __forceinline__ float tail_finish(TAIL32_PARAMS, const float b4) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int sidx = 16 + r;
        ys[r & 3] = fmaf(w4[sidx >> 2][sidx & 3], lrelu1(acc3[1][r]), ys[r & 3]);
    }
    float y = (ys[0] + ys[1]) + (ys[2] + ys[3]);
    y += __shfl_xor(y, 32);
    return y + b4;
}
