// lidf_loss.hip — the training steps' ground truth and losses (LIDF.compute_gt, models/pipeline.py:298-336, the
// training part of LIDF.compute_loss, :468-566, and of RefineNet.compute_loss, :760-840) on the compact ray-major
// pair list:
//   lidf_pair_labels_kernel        gt_pos gather, per-pair inside test, label-selected pair of every ray, label count,
//                                  pixel -> ray table
//   lidf_loss_kernel               per ray: L1 position term, log-softmax terms of its labelled pairs, surface normal
//                                  and smoothness terms at its own pixel, the metrics; per-block partial sums
//   lidf_loss_final_kernel         the partial sums in a fixed order -> the eight (stage 2: six) scalars of loss_dict
//   <.., EVAL = true> of the two    the evaluation flavour ('valid' / 'test', :571-650, :843-919): xyz_corrupt_flat as
//                                  the base cloud, no stored terms unless asked for, the nine ClearGrasp statistics
//                                  -> 17 (stage 2: 15) scalars; lidf_eval_depth_images_kernel feeds the bs == 1 branch
//   <.., EVAL = true, FRAMES = true> the same per frame of a batch (lidf_*_eval_loss_frames_f32): frame b owns the
//                                  rays [s_b, s_{b+1}) of the grouped ray list (a lower bound over ray_bid, taken on
//                                  the device), its blocks of 256 rays count from s_b, and row b of loss [B, 17 | 15]
//                                  is what the bs == 1 call on that frame alone gives, bit for bit
//   lidf_loss_backward_kernel      per ray: d loss_net / d pred_pos (a gather over its own, its left and its
//                                  upper pixel's normals) and d loss_net / d logits of its pairs (closed form)
// The three loss kernels are templates on PAIRS: <true> is stage 1 (lidf_stage1_loss_*), <false> is stage 2
// (lidf_refine_loss_*: pred_pos is pred_pos_refine, no ray-termination term and no acc, no pair list is read — a ray
// without pairs is an ordinary ray — and loss_dict has six entries).
// No V x R mask, no image-sized normal map (lidf_normal_map_kernel writes the two maps on request only), no float
// atomics: every sum has a fixed order, so losses and gradients are bit-identical from run to run.
// Hard-negative mining — the top-k means of the unreduced terms written here, and the w_* the backward reads — is
// torch.topk on the host side by default and lidf_select.hip (lidf_stage1_hard_neg_f32 / lidf_refine_hard_neg_f32) on
// request: that file rewrites loss[0..4] (stage 2: loss[0..3]) after lidf_loss_final_kernel.
#include "lidf_launch.h"

namespace {

constexpr int LOSS_BLOCK = 256;
constexpr int NSUM = 9;
enum { S_POS, S_PROB, S_SURF, S_DX, S_DY, S_ACC, S_ERR, S_ELEM, S_ANGLE };
constexpr int NMET = 9;   // evaluation flavour: depth_metric_terms' sums follow the NSUM sums of the training flavour

// G lanes per ray (a wavefront takes 64 / G rays): a geometry-derived frame has a handful of pairs per ray.
template <int G>
__global__ void lidf_pair_labels_kernel(const float* __restrict__ xyz, const int* __restrict__ ray_bid,
                                        const int* __restrict__ ray_flat, long long hw,
                                        const int* __restrict__ off, const int* __restrict__ pair_vox,
                                        const float* __restrict__ vbound, long long R, long long P,
                                        float* __restrict__ gt_pos, long long* __restrict__ label,
                                        float* __restrict__ labelf, long long* __restrict__ maxid,
                                        int* __restrict__ n_label, int* __restrict__ pix2ray) {
    __shared__ int block_cnt;
    if (threadIdx.x == 0) block_cnt = 0;
    __syncthreads();
    const int lane = threadIdx.x & (G - 1);
    const long long r = ((long long)blockIdx.x * blockDim.x + threadIdx.x) / G;
    const bool live = r < R;
    int cnt = 0, first = 0x7fffffff, beg = 0, end = 0;
    long long q = 0;
    float x = 0.f, y = 0.f, z = 0.f;
    if (live) {
        q = (long long)ray_bid[r] * hw + ray_flat[r];
        x = xyz[3 * q], y = xyz[3 * q + 1], z = xyz[3 * q + 2];
        beg = off[r], end = off[r + 1];
        for (int i = beg + lane; i < end; i += G) {
            float vb[6];
            const float* src = vbound + 6 * (size_t)pair_vox[i];
#pragma unroll
            for (int k = 0; k < 6; ++k) vb[k] = src[k];
            const bool in = inside_box(x, y, z, vb);
            label[i] = in ? 1 : 0;
            labelf[i] = in ? 1.f : 0.f;
            if (in) {
                ++cnt;
                first = first < i ? first : i;
            }
        }
    }
#pragma unroll
    for (int s = G / 2; s >= 1; s >>= 1) {
        const int of = __shfl_xor(first, s);
        cnt += __shfl_xor(cnt, s);
        first = of < first ? of : first;
    }
    if (live && lane == 0) {
        gt_pos[3 * r] = x, gt_pos[3 * r + 1] = y, gt_pos[3 * r + 2] = z;
        // scatter_max of the 0 / 1 labels (models/pipeline.py:445): the first labelled pair, the ray's first pair
        // when none is labelled (every value ties at 0), P for a ray without pairs. Inside a ray the voxels ascend,
        // so the lowest ray-major index is the lowest index of the reference's voxel-major order as well
        maxid[r] = end <= beg ? P : (long long)(first < end ? first : beg);
        if (pix2ray) pix2ray[q] = (int)r;
        if (cnt) atomicAdd(&block_cnt, cnt);   // (integer: the order does not matter)
    }
    __syncthreads();
    if (threadIdx.x == 0 && block_cnt) atomicAdd(n_label, block_cnt);
}

// One pixel's terms of point_utils.get_surface_normal (utils/point_utils.py:210-235) on the frame with the sampled
// pixels replaced by `pos`: dx = right - self, dy = below - self (the constant 0 in the last column / row),
// n = dx x dy, a = n / (|n| + 1e-8).
struct PixNormal {
    float dx[3], dy[3], n[3], a[3], nrm;
};

__device__ __forceinline__ void frame_point(const LossArgs& A, const float* __restrict__ pos, long long q, float* p) {
    const int t = A.pix2ray[q];
    const float* src = t >= 0 ? pos + 3 * (size_t)t : A.xyz + 3 * (size_t)q;
    p[0] = src[0], p[1] = src[1], p[2] = src[2];
}

__device__ __forceinline__ void pix_normal(const LossArgs& A, const float* __restrict__ pos, long long base, int y,
                                           int x, PixNormal& o) {
    const long long q = base + (long long)y * A.W + x;
    float p0[3], pr[3], pb[3];
    frame_point(A, pos, q, p0);
    const bool hx = x < A.W - 1, hy = y < A.H - 1;
    if (hx) frame_point(A, pos, q + 1, pr);
    if (hy) frame_point(A, pos, q + A.W, pb);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        o.dx[k] = hx ? pr[k] - p0[k] : 0.f;
        o.dy[k] = hy ? pb[k] - p0[k] : 0.f;
    }
    o.n[0] = o.dx[1] * o.dy[2] - o.dx[2] * o.dy[1];
    o.n[1] = o.dx[2] * o.dy[0] - o.dx[0] * o.dy[2];
    o.n[2] = o.dx[0] * o.dy[1] - o.dx[1] * o.dy[0];
    o.nrm = sqrtf(o.n[0] * o.n[0] + o.n[1] * o.n[1] + o.n[2] * o.n[2]);
    const float s = o.nrm + 1e-8f;
#pragma unroll
    for (int k = 0; k < 3; ++k) o.a[k] = o.n[k] / s;
}

// F.cosine_similarity(a, b, dim=-1, eps=1e-8) as torch >= 1.12 defines it: both vectors are divided by their norms,
// clamped from below at eps, before the product is summed. Returns the value and the clamped norms.
__device__ __forceinline__ float cosine(const float* a, const float* b, float& na, float& nb, float* bh) {
    const float ra = sqrtf(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
    const float rb = sqrtf(b[0] * b[0] + b[1] * b[1] + b[2] * b[2]);
    na = fmaxf(ra, 1e-8f), nb = fmaxf(rb, 1e-8f);
    float c = 0.f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        bh[k] = b[k] / nb;
        c += (a[k] / na) * bh[k];
    }
    return c;
}

// First ray of frame b in the grouped ray list: the lowest i in [0, R] with ray_bid[i] >= b (b = B gives R). On a
// list that is not grouped the answer is still an index in [0, R].
__device__ __forceinline__ long long frame_start(const int* __restrict__ ray_bid, long long R, int b) {
    long long lo = 0, hi = R;
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (ray_bid[mid] < b) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// EVAL: the exp_type != 'train' flavour (:571-618, :843-889). A.xyz is then xyz_corrupt_flat (:497), the unreduced
// terms are stored only where their pointer is set (hard-negative mining), ray_lse is not stored (no backward), and
// the terms of the nine statistics over the rays with nonzero ground truth (the bs != 1 branch: pred = pred_pos z,
// gt = gt_pos z) join the partial sums.
// FRAMES (with EVAL): grid (ceil(hw / 256), B) — a ray is a distinct pixel, so no frame has more than hw rays.
// Block j of frame b takes the rays s_b + 256 j ... of that frame and writes partial row (b, j); a block at or
// beyond the frame's ceil(R_b / 256) leaves without touching memory. Stage 1 carries one more sum, the number of
// labelled pairs of the ray (integer-valued, exact in double): the frame's own n_label.
template <bool PAIRS, bool EVAL, bool FRAMES = false>
__global__ __launch_bounds__(LOSS_BLOCK) void lidf_loss_kernel(const LossArgs A) {
    static_assert(EVAL || !FRAMES, "the per-frame form is the evaluation flavour's");
    constexpr int NS = EVAL ? NSUM + NMET : NSUM;
    constexpr int NP = NS + (FRAMES && PAIRS ? 1 : 0);
    long long r = (long long)blockIdx.x * LOSS_BLOCK + threadIdx.x;
    long long r_end = A.R;
    if constexpr (FRAMES) {
        __shared__ long long s_range[2];
        if (threadIdx.x < 2) s_range[threadIdx.x] = frame_start(A.ray_bid, A.R, (int)blockIdx.y + (int)threadIdx.x);
        __syncthreads();
        r_end = s_range[1];
        if (s_range[0] + (long long)blockIdx.x * LOSS_BLOCK >= r_end) return;   // (the whole block)
        r += s_range[0];
    }
    double v[NP];
#pragma unroll
    for (int k = 0; k < NP; ++k) v[k] = 0.0;
    if (r < r_end) {
        // position term and the L2 error over rays whose ground truth is not the zero-depth point (:560-566)
        float g[3], d[3];
        float pz = 0.f;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            g[k] = A.gt_pos[3 * r + k];
            pz = A.pred_pos[3 * r + k];   // (after the loop: the predicted depth)
            d[k] = pz - g[k];
        }
        const float l1 = fabsf(d[0]) + fabsf(d[1]) + fabsf(d[2]);
        if (!EVAL || A.pos_un) A.pos_un[r] = l1 / 3.f;
        v[S_POS] = l1;
        if (fabsf(g[0]) + fabsf(g[1]) + fabsf(g[2]) != 0.f) {
            v[S_ERR] = sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
            v[S_ELEM] = 1.0;
            if constexpr (EVAL) depth_metric_terms(g[2], pz, v + NSUM);
        }
        // log-softmax over the ray's pairs, taken at its labelled pairs (:482-484); arg-max of the softmax with
        // lidf_ray_reduce_kernel's rule (first of equal values, P when nothing compares greater than -inf)
        if constexpr (PAIRS) {
            const int beg = A.pair_off[r], end = A.pair_off[r + 1];
            float m = -INFINITY;
            for (int i = beg; i < end; ++i) m = fmaxf(m, A.logit[i]);
            float s = 0.f;
            for (int i = beg; i < end; ++i) s += expf(A.logit[i] - m);
            const float ls = logf(s);
            float bv = -INFINITY, psum = 0.f;
            int bi = 0x7fffffff;
            for (int i = beg; i < end; ++i) {
                const float z = A.logit[i] - m;
                const float sm = expf(z) / s;
                if (sm > bv) bv = sm, bi = i;
                float l = -INFINITY;
                if (A.label[i] != 0) {
                    l = -(z - ls);
                    psum += l;
                    if constexpr (FRAMES) v[NS] += 1.0;
                }
                if (!EVAL || A.prob_un) A.prob_un[i] = l;
            }
            if constexpr (!EVAL) A.ray_lse[2 * r] = m, A.ray_lse[2 * r + 1] = ls;
            v[S_PROB] = psum;
            const long long pred_label = (end <= beg || bi >= end) ? A.P : (long long)bi;
            v[S_ACC] = pred_label == A.gt_maxid[r] ? 1.0 : 0.0;
        }
        // surface normal and smoothness terms at the ray's own pixel (:494-539)
        const int b = A.ray_bid[r], f = A.ray_flat[r];
        const int y = f / A.W, x = f - y * A.W;
        PixNormal np, ng;
        pix_normal(A, A.pred_pos, (long long)b * A.hw, y, x, np);
        pix_normal(A, A.gt_pos, (long long)b * A.hw, y, x, ng);
        float na, nb, bh[3];
        const float c = cosine(np.a, ng.a, na, nb, bh);
        const float dist = (1.f - c) / 2.f;
        const float cc = c < -1.f ? -1.f : (c > 1.f ? 1.f : c);   // (a NaN stays a NaN, as in torch.clamp)
        const float dxd = np.dx[0] * np.dx[0] + np.dx[1] * np.dx[1] + np.dx[2] * np.dx[2];
        const float dyd = np.dy[0] * np.dy[0] + np.dy[1] * np.dy[1] + np.dy[2] * np.dy[2];
        if (!EVAL || A.surf_dist) A.surf_dist[r] = dist, A.dx_dist[r] = dxd, A.dy_dist[r] = dyd;
        v[S_SURF] = dist, v[S_DX] = dxd, v[S_DY] = dyd, v[S_ANGLE] = acosf(cc);
    }
    // stage 1 of the means: the block's sums (wavefront butterflies, then the four wavefronts in order)
    __shared__ double part[LOSS_BLOCK / 64][NP];
    const int wv = threadIdx.x >> 6, ln = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < NP; ++k) {
        const double t = wave_sum(v[k]);
        if (ln == 0) part[wv][k] = t;
    }
    __syncthreads();
    if (threadIdx.x < NP) {
        double t = 0.0;
#pragma unroll
        for (int i = 0; i < LOSS_BLOCK / 64; ++i) t += part[i][threadIdx.x];
        const size_t row = FRAMES ? (size_t)blockIdx.y * gridDim.x + blockIdx.x : (size_t)blockIdx.x;
        A.partial[row * NP + threadIdx.x] = t;
    }
}

// Stage 2: wavefront k sums quantity k over the blocks (lane-strided, then a butterfly: a fixed order), thread 0
// forms loss_dict = {pos_loss, prob_loss, surf_norm_loss, smooth_loss, loss_net, acc, err, angle_err} (:542-566);
// stage 2: {pos_loss, surf_norm_loss, smooth_loss, loss_net, err, angle_err} (:823-840, :898-905).
// EVAL: every wavefront takes a second quantity, and the nine statistics follow in loss_dict's order (:639-649,
// :906-917) — from the rays' sums, or copied from A.metrics (the resized frame of the bs == 1 branch).
// FRAMES: one workgroup per frame; nblk arrives as the partial rows per frame (the launch's ceil(hw / 256)) and
// becomes the frame's own ceil(R_b / 256), R its R_b, the label count its own sum, A.metrics / A.loss its rows of
// [B, 10] / [B, 17 | 15]. A frame without a ray has no loss_dict (the reference returns early): its row is NaN.
template <bool PAIRS, bool EVAL, bool FRAMES = false>
__global__ __launch_bounds__(64 * NSUM) void lidf_loss_final_kernel(const LossArgs A, int nblk) {
    constexpr int NS = EVAL ? NSUM + NMET : NSUM;
    constexpr int NP = NS + (FRAMES && PAIRS ? 1 : 0);
    __shared__ double tot[NP];
    const int wv = threadIdx.x >> 6, ln = threadIdx.x & 63;
    const double* partial = A.partial;
    long long n_rays = A.R;
    float* loss = A.loss;
    const float* metrics = A.metrics;
    if constexpr (FRAMES) {
        __shared__ long long s_range[2];
        if (threadIdx.x < 2) s_range[threadIdx.x] = frame_start(A.ray_bid, A.R, (int)blockIdx.x + (int)threadIdx.x);
        __syncthreads();
        n_rays = s_range[1] - s_range[0];
        constexpr int NL = (PAIRS ? 8 : 6) + NMET;
        loss += (size_t)blockIdx.x * NL;
        if (n_rays <= 0) {
            if (threadIdx.x < NL) loss[threadIdx.x] = __builtin_nanf("");
            return;
        }
        partial += (size_t)blockIdx.x * nblk * NP;
        metrics += (size_t)blockIdx.x * 10;
        // (a grouped list has R_b <= hw; the clamp keeps an ungrouped one inside the frame's partial rows)
        const long long own = (n_rays + LOSS_BLOCK - 1) / LOSS_BLOCK;
        nblk = own < nblk ? (int)own : nblk;
    }
    auto total = [&](int k) {
        double t = 0.0;
        for (int i = ln; i < nblk; i += 64) t += partial[(size_t)i * NP + k];
        t = wave_sum(t);
        if (ln == 0) tot[k] = t;
    };
    total(wv);
    if constexpr (EVAL) total(wv + NSUM);
    if constexpr (FRAMES && PAIRS) {
        if (wv == 0) total(NS);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double R = (double)n_rays;
        const float pos = (float)(tot[S_POS] / (3.0 * R));
        const float surf = (float)(tot[S_SURF] / R);
        const float smooth = (float)(tot[S_DX] / R) + (float)(tot[S_DY] / R);
        const float err = tot[S_ELEM] == 0.0 ? 0.f : (float)(tot[S_ERR] / tot[S_ELEM]);
        const float angle = (float)(tot[S_ANGLE] / R) / 3.14159265358979323846f * 180.f;
        if constexpr (PAIRS) {
            double L;
            if constexpr (FRAMES) L = tot[NS];
            else L = (double)*A.n_label;
            const float prob = (float)(tot[S_PROB] / L);   // L == 0: 0 / 0 = NaN, torch.mean of an empty tensor
            float net = A.pos_w * pos + A.prob_w * prob;
            if (A.surf_on) net += A.surf_w * surf;
            if (A.smooth_on) net += A.smooth_w * smooth;
            loss[0] = pos, loss[1] = prob, loss[2] = surf, loss[3] = smooth, loss[4] = net;
            loss[5] = (float)(tot[S_ACC] / R);
            loss[6] = err;
            loss[7] = angle;
        } else {
            float net = A.pos_w * pos;
            if (A.surf_on) net += A.surf_w * surf;
            if (A.smooth_on) net += A.smooth_w * smooth;
            loss[0] = pos, loss[1] = surf, loss[2] = smooth, loss[3] = net, loss[4] = err, loss[5] = angle;
        }
        if constexpr (EVAL) {
            float* out = loss + (PAIRS ? 8 : 6);
            if (metrics) {
#pragma unroll
                for (int i = 0; i < NMET; ++i) out[i] = metrics[i];
            } else {
                depth_metric_stats(tot + NSUM, tot[S_ELEM], out);
            }
        }
    }
}

// The bs == 1 branch's two depth images (:579-597), which lidf_depth_metrics_kernel resizes: z of the ground-truth
// frame, and z of the base cloud with the queried pixels replaced by pred_pos.
__global__ void lidf_eval_depth_images_kernel(const LossArgs A, const float* __restrict__ xyz_gt,
                                              float* __restrict__ pred_img, float* __restrict__ gt_img) {
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= A.hw) return;
    const int t = A.pix2ray[q];
    pred_img[q] = t >= 0 ? A.pred_pos[3 * (size_t)t + 2] : A.xyz[3 * (size_t)q + 2];
    gt_img[q] = xyz_gt[3 * (size_t)q + 2];
}

// The same two images for every frame of a batch ([B, hw] each): pix2ray holds the batch's ray numbers.
__global__ void lidf_eval_depth_images_frames_kernel(const LossArgs A, const float* __restrict__ xyz_gt,
                                                     float* __restrict__ pred_img, float* __restrict__ gt_img) {
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= (long long)A.B * A.hw) return;
    const int t = A.pix2ray[q];
    pred_img[q] = t >= 0 ? A.pred_pos[3 * (size_t)t + 2] : A.xyz[3 * (size_t)q + 2];
    gt_img[q] = xyz_gt[3 * (size_t)q + 2];
}

// d loss_net / d (dx, dy) of the sampled pixel (y, x) of ray rj, through its normal's cosine term (weight cs on
// (1 - cos) / 2) and its smoothness terms (weights cdx, cdy on |dx|^2, |dy|^2). The last column's dx and the last
// row's dy are constants: their gradients are returned as 0.
__device__ __forceinline__ void pix_grad(const LossArgs& A, long long base, int y, int x, float cs, float cdx,
                                         float cdy, float* gdx, float* gdy) {
    PixNormal np;
    pix_normal(A, A.pred_pos, base, y, x, np);
    float gn[3] = {0.f, 0.f, 0.f};
    if (cs != 0.f) {
        PixNormal ng;
        pix_normal(A, A.gt_pos, base, y, x, ng);
        float na, nb, bh[3];
        cosine(np.a, ng.a, na, nb, bh);
        // cos = sum_k (a_k / na) bh_k with na = max(|a|, eps): the norm's own derivative a / |a| (0 at a = 0) is not
        // clamped, the divisor is
        const float ra = sqrtf(np.a[0] * np.a[0] + np.a[1] * np.a[1] + np.a[2] * np.a[2]);
        const float t = (np.a[0] * bh[0] + np.a[1] * bh[1] + np.a[2] * bh[2]) / (na * na);
        const float gc = -0.5f * cs;
        float ga[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) ga[k] = gc * (bh[k] / na - (ra > 0.f ? t * (np.a[k] / ra) : 0.f));
        // a = n / (|n| + 1e-8)
        const float s = np.nrm + 1e-8f;
        const float ng_dot = np.n[0] * ga[0] + np.n[1] * ga[1] + np.n[2] * ga[2];
#pragma unroll
        for (int k = 0; k < 3; ++k)
            gn[k] = ga[k] / s - (np.nrm > 0.f ? np.n[k] * (ng_dot / (np.nrm * s * s)) : 0.f);
    }
    // n = dx x dy: d/d dx = dy x gn, d/d dy = gn x dx
    const bool hx = x < A.W - 1, hy = y < A.H - 1;
    const float cx[3] = {np.dy[1] * gn[2] - np.dy[2] * gn[1], np.dy[2] * gn[0] - np.dy[0] * gn[2],
                         np.dy[0] * gn[1] - np.dy[1] * gn[0]};
    const float cy[3] = {gn[1] * np.dx[2] - gn[2] * np.dx[1], gn[2] * np.dx[0] - gn[0] * np.dx[2],
                         gn[0] * np.dx[1] - gn[1] * np.dx[0]};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        gdx[k] = hx ? cx[k] + 2.f * cdx * np.dx[k] : 0.f;
        gdy[k] = hy ? cy[k] + 2.f * cdy * np.dy[k] : 0.f;
    }
}

__device__ __forceinline__ void pix_weights(const LossArgs& A, long long rj, float up, float invR, float& cs,
                                            float& cdx, float& cdy) {
    cs = A.surf_on ? up * A.surf_w * (A.w_surf ? A.w_surf[rj] : invR) : 0.f;
    cdx = A.smooth_on ? up * A.smooth_w * (A.w_dx ? A.w_dx[rj] : invR) : 0.f;
    cdy = A.smooth_on ? up * A.smooth_w * (A.w_dy ? A.w_dy[rj] : invR) : 0.f;
}

template <bool PAIRS>
__global__ __launch_bounds__(LOSS_BLOCK) void lidf_loss_backward_kernel(const LossArgs A) {
    const long long r = (long long)blockIdx.x * LOSS_BLOCK + threadIdx.x;
    if (r >= A.R) return;
    const float up = *A.g_loss_net;
    const float invR = 1.f / (float)A.R;
    if constexpr (PAIRS) {
        const int L = *A.n_label;
        const float invL = L > 0 ? 1.f / (float)L : 0.f;   // (no labelled pair: the empty mean reaches no logit)
        // logits: sum over the ray's labelled pairs j of w_j (softmax_i - [i == j])
        const int beg = A.pair_off[r], end = A.pair_off[r + 1];
        const float m = A.ray_lse[2 * r], ls = A.ray_lse[2 * r + 1];
        float wsum = 0.f;
        for (int i = beg; i < end; ++i)
            if (A.label[i] != 0) wsum += A.w_prob ? A.w_prob[i] : invL;
        const float kp = up * A.prob_w;
        for (int i = beg; i < end; ++i) {
            const float sm = expf((A.logit[i] - m) - ls);
            const float wl = A.label[i] != 0 ? (A.w_prob ? A.w_prob[i] : invL) : 0.f;
            A.g_logit[i] = kp * (wsum * sm - wl);
        }
    }
    // position term: sign(pred - gt) / 3 per coordinate of the ray's mean
    const float kpos = up * A.pos_w * (A.w_pos ? A.w_pos[r] : invR) / 3.f;
    float g[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float d = A.pred_pos[3 * r + k] - A.gt_pos[3 * r + k];
        g[k] = d > 0.f ? kpos : (d < 0.f ? -kpos : (d == 0.f ? 0.f : d * kpos));   // (NaN propagates)
    }
    if (A.surf_on || A.smooth_on) {
        // the ray's point enters its own pixel's dx and dy with -1, its left pixel's dx and its upper pixel's dy
        // with +1 (where those pixels are sampled rays: only their normals are in the loss)
        const int b = A.ray_bid[r], f = A.ray_flat[r];
        const int y = f / A.W, x = f - y * A.W;
        const long long base = (long long)b * A.hw;
        float cs, cdx, cdy, gdx[3], gdy[3];
        pix_weights(A, r, up, invR, cs, cdx, cdy);
        pix_grad(A, base, y, x, cs, cdx, cdy, gdx, gdy);
#pragma unroll
        for (int k = 0; k < 3; ++k) g[k] = g[k] - gdx[k] - gdy[k];
        const int tl = x > 0 ? A.pix2ray[base + f - 1] : -1;
        if (tl >= 0) {
            pix_weights(A, tl, up, invR, cs, cdx, cdy);
            pix_grad(A, base, y, x - 1, cs, cdx, cdy, gdx, gdy);
#pragma unroll
            for (int k = 0; k < 3; ++k) g[k] += gdx[k];
        }
        const int tu = y > 0 ? A.pix2ray[base + f - A.W] : -1;
        if (tu >= 0) {
            pix_weights(A, tu, up, invR, cs, cdx, cdy);
            pix_grad(A, base, y - 1, x, cs, cdx, cdy, gdx, gdy);
#pragma unroll
            for (int k = 0; k < 3; ++k) g[k] += gdy[k];
        }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) A.g_pred_pos[3 * r + k] = g[k];
}

// data_dict['gt_surf_norm_img'] / ['pred_surf_norm_img'] ([B,3,H,W], visualisation only): every pixel's normal.
__global__ void lidf_normal_map_kernel(const LossArgs A, float* __restrict__ gt_img, float* __restrict__ pred_img) {
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= (long long)A.B * A.hw) return;
    const long long b = q / A.hw, f = q - b * A.hw;
    const int y = (int)(f / A.W), x = (int)(f - (long long)y * A.W);
    PixNormal o;
    if (gt_img) {
        pix_normal(A, A.gt_pos, b * A.hw, y, x, o);
#pragma unroll
        for (int k = 0; k < 3; ++k) gt_img[(b * 3 + k) * A.hw + f] = o.a[k];
    }
    if (pred_img) {
        pix_normal(A, A.pred_pos, b * A.hw, y, x, o);
#pragma unroll
        for (int k = 0; k < 3; ++k) pred_img[(b * 3 + k) * A.hw + f] = o.a[k];
    }
}

}  // namespace

extern "C" hipError_t lidf_launch_pair_labels(const float* xyz, const int* ray_bid, const int* ray_flat, long long hw,
                                              const int* pair_off, const int* pair_vox, const float* vbound,
                                              long long R, long long P, float* gt_pos, long long* label,
                                              float* labelf, long long* maxid, int* n_label, int* pix2ray,
                                              hipStream_t st) {
    if (R <= 0) return hipSuccess;
    constexpr int G = 8;
    const long long blocks = (R * G + LOSS_BLOCK - 1) / LOSS_BLOCK;
    hipLaunchKernelGGL(lidf_pair_labels_kernel<G>, dim3((unsigned)blocks), dim3(LOSS_BLOCK), 0, st, xyz, ray_bid,
                       ray_flat, hw, pair_off, pair_vox, vbound, R, P, gt_pos, label, labelf, maxid, n_label, pix2ray);
    return hipGetLastError();
}

extern "C" size_t lidf_stage1_loss_partial_bytes(long long R) {
    const long long blocks = R > 0 ? (R + LOSS_BLOCK - 1) / LOSS_BLOCK : 0;
    return (size_t)blocks * NSUM * sizeof(double);
}

extern "C" hipError_t lidf_launch_stage1_loss(const LossArgs& a, float* gt_img, float* pred_img, hipStream_t st) {
    if (a.R <= 0) return hipSuccess;
    const int blocks = (int)((a.R + LOSS_BLOCK - 1) / LOSS_BLOCK);
    hipLaunchKernelGGL((lidf_loss_kernel<true, false>), dim3((unsigned)blocks), dim3(LOSS_BLOCK), 0, st, a);
    hipLaunchKernelGGL((lidf_loss_final_kernel<true, false>), dim3(1), dim3(64 * NSUM), 0, st, a, blocks);
    if (gt_img || pred_img) {
        const long long n = (long long)a.B * a.hw;
        hipLaunchKernelGGL(lidf_normal_map_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a, gt_img,
                           pred_img);
    }
    return hipGetLastError();
}

// The evaluation flavour of either stage (pairs: stage 1), two launches.
extern "C" size_t lidf_eval_loss_partial_bytes(long long R) {
    const long long blocks = R > 0 ? (R + LOSS_BLOCK - 1) / LOSS_BLOCK : 0;
    return (size_t)blocks * (NSUM + NMET) * sizeof(double);
}

extern "C" hipError_t lidf_launch_eval_loss(const LossArgs& a, int pairs, hipStream_t st) {
    if (a.R <= 0) return hipSuccess;
    const int blocks = (int)((a.R + LOSS_BLOCK - 1) / LOSS_BLOCK);
    if (pairs) {
        hipLaunchKernelGGL((lidf_loss_kernel<true, true>), dim3((unsigned)blocks), dim3(LOSS_BLOCK), 0, st, a);
        hipLaunchKernelGGL((lidf_loss_final_kernel<true, true>), dim3(1), dim3(64 * NSUM), 0, st, a, blocks);
    } else {
        hipLaunchKernelGGL((lidf_loss_kernel<false, true>), dim3((unsigned)blocks), dim3(LOSS_BLOCK), 0, st, a);
        hipLaunchKernelGGL((lidf_loss_final_kernel<false, true>), dim3(1), dim3(64 * NSUM), 0, st, a, blocks);
    }
    return hipGetLastError();
}

extern "C" hipError_t lidf_launch_eval_depth_images(const LossArgs& a, const float* xyz_gt, float* pred_img,
                                                    float* gt_img, hipStream_t st) {
    if (a.hw <= 0) return hipSuccess;
    hipLaunchKernelGGL(lidf_eval_depth_images_kernel, dim3((unsigned)((a.hw + 255) / 256)), dim3(256), 0, st, a, xyz_gt,
                       pred_img, gt_img);
    return hipGetLastError();
}

// The per-frame form: ceil(hw / 256) partial rows of 18 (stage 1: 19) doubles per frame, two launches.
extern "C" size_t lidf_eval_loss_frames_partial_bytes(int B, long long hw, int pairs) {
    if (B <= 0 || hw <= 0) return 0;
    const long long blocks = (hw + LOSS_BLOCK - 1) / LOSS_BLOCK;
    return (size_t)B * blocks * (NSUM + NMET + (pairs ? 1 : 0)) * sizeof(double);
}

extern "C" hipError_t lidf_launch_eval_loss_frames(const LossArgs& a, int pairs, hipStream_t st) {
    if (a.R <= 0 || a.B <= 0 || a.hw <= 0) return hipSuccess;
    const int blocks = (int)((a.hw + LOSS_BLOCK - 1) / LOSS_BLOCK);
    const dim3 grid((unsigned)blocks, (unsigned)a.B);
    if (pairs) {
        hipLaunchKernelGGL((lidf_loss_kernel<true, true, true>), grid, dim3(LOSS_BLOCK), 0, st, a);
        hipLaunchKernelGGL((lidf_loss_final_kernel<true, true, true>), dim3((unsigned)a.B), dim3(64 * NSUM), 0, st, a,
                           blocks);
    } else {
        hipLaunchKernelGGL((lidf_loss_kernel<false, true, true>), grid, dim3(LOSS_BLOCK), 0, st, a);
        hipLaunchKernelGGL((lidf_loss_final_kernel<false, true, true>), dim3((unsigned)a.B), dim3(64 * NSUM), 0, st, a,
                           blocks);
    }
    return hipGetLastError();
}

extern "C" hipError_t lidf_launch_eval_depth_images_frames(const LossArgs& a, const float* xyz_gt, float* pred_img,
                                                           float* gt_img, hipStream_t st) {
    const long long n = (long long)a.B * a.hw;
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(lidf_eval_depth_images_frames_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a,
                       xyz_gt, pred_img, gt_img);
    return hipGetLastError();
}

extern "C" hipError_t lidf_launch_stage1_loss_backward(const LossArgs& a, hipStream_t st) {
    if (a.R <= 0) return hipSuccess;
    hipLaunchKernelGGL(lidf_loss_backward_kernel<true>, dim3((unsigned)((a.R + LOSS_BLOCK - 1) / LOSS_BLOCK)),
                       dim3(LOSS_BLOCK), 0, st, a);
    return hipGetLastError();
}

// Stage 2 (RefineNet.compute_loss): a.pred_pos is pred_pos_refine; the pair fields of `a` are not read.
extern "C" hipError_t lidf_launch_refine_loss(const LossArgs& a, float* pred_img, hipStream_t st) {
    if (a.R <= 0) return hipSuccess;
    const int blocks = (int)((a.R + LOSS_BLOCK - 1) / LOSS_BLOCK);
    hipLaunchKernelGGL((lidf_loss_kernel<false, false>), dim3((unsigned)blocks), dim3(LOSS_BLOCK), 0, st, a);
    hipLaunchKernelGGL((lidf_loss_final_kernel<false, false>), dim3(1), dim3(64 * NSUM), 0, st, a, blocks);
    if (pred_img) {
        const long long n = (long long)a.B * a.hw;
        hipLaunchKernelGGL(lidf_normal_map_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a,
                           (float*)nullptr, pred_img);
    }
    return hipGetLastError();
}

extern "C" hipError_t lidf_launch_refine_loss_backward(const LossArgs& a, hipStream_t st) {
    if (a.R <= 0) return hipSuccess;
    hipLaunchKernelGGL(lidf_loss_backward_kernel<false>, dim3((unsigned)((a.R + LOSS_BLOCK - 1) / LOSS_BLOCK)),
                       dim3(LOSS_BLOCK), 0, st, a);
    return hipGetLastError();
}
