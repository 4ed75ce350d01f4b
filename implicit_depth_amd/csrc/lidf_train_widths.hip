// lidf_train_widths.hip — the two adjoints the stage-1 training step needs at widths other than the shipped
// configuration (implicit_depth_amd/generic.py, query_train):
//   * the adjoint of lidf_roi_align_kernel (lidf_aux.hip) at any channel count and output size, as a gather:
//     a pixel -> ray table, then one thread per (feature pixel, 8 channels) that visits the rays centred within
//     reach and sums weight x gradient — no float atomics;
//   * the adjoint of the two gathered terms of lidf_linear_gather2_f32 at any width that is a multiple of 4:
//     sums over contiguous row ranges (lidf_launch_seg_sum_ray, lidf_train.hip, takes any width already) and sums
//     by an arbitrary row index — lidf_train.hip's stable counting sort (lidf_launch_sort_idx), chunk sums of
//     SEGW_CH sorted rows and an in-order final pass, the plan of lidf_launch_seg_sum_idx without its 256 columns.
// The fixed-width launchers of lidf_train.hip are not touched: the shipped configuration runs what it ran.
#include "lidf_launch.h"

// ------------------------------------------------------------------------------------------------------------------
// RoIAlign backward
// ------------------------------------------------------------------------------------------------------------------
// Rays of one chunk per pixel: cnt[(b * H + y) * W + x] (zeroed by the launcher). A ray whose frame or pixel lies
// outside the image is left out here and in the fill pass (the forward does not check them; an adjoint that writes
// must).
__global__ void __launch_bounds__(256) lidf_roiw_count_kernel(const int* __restrict__ ray_pix,
                                                              const int* __restrict__ ray_bid, long long r0,
                                                              long long r1, int B, int H, int W,
                                                              int* __restrict__ cnt) {
    const long long r = r0 + (long long)blockIdx.x * 256 + threadIdx.x;
    if (r >= r1) return;
    const int qx = ray_pix[2 * r], qy = ray_pix[2 * r + 1], b = ray_bid[r];
    if (qx < 0 || qx >= W || qy < 0 || qy >= H || b < 0 || b >= B) return;
    atomicAdd(cnt + ((size_t)b * H + qy) * W + qx, 1);
}

// list[start[pix] .. start[pix + 1]) = the chunk's rays on that pixel (chunk-relative). The slots of a pixel are
// handed out by an integer atomic that counts cnt back down to zero: with one ray per pixel the table is the same in
// every run, with several the order inside a pixel is not fixed.
__global__ void __launch_bounds__(256) lidf_roiw_fill_kernel(const int* __restrict__ ray_pix,
                                                             const int* __restrict__ ray_bid, long long r0,
                                                             long long r1, int B, int H, int W,
                                                             int* __restrict__ cnt, const int* __restrict__ start,
                                                             int* __restrict__ list) {
    const long long r = r0 + (long long)blockIdx.x * 256 + threadIdx.x;
    if (r >= r1) return;
    const int qx = ray_pix[2 * r], qy = ray_pix[2 * r + 1], b = ray_bid[r];
    if (qx < 0 || qx >= W || qy < 0 || qy >= H || b < 0 || b >= B) return;
    const size_t pix = ((size_t)b * H + qy) * W + qx;
    const int slot = atomicSub(cnt + pix, 1) - 1;
    list[start[pix] + slot] = (int)(r - r0);
}

// The weight one axis of bin `p` puts on pixel coordinate `at`: the sum over the bin's `g` samples of the linear
// tap weights of bilinear() (lidf_aux.hip) that land on `at`. rs: the box's start (corner - 0.5), bin: the bin size,
// n: the image extent. The forward's outside test never fires on a clamped box (samples lie in [-0.5, n - 1.5]).
__device__ __forceinline__ float roiw_axis_weight(float rs, float bin, int g, int p, int at, int n) {
    float w = 0.f;
    for (int i = 0; i < g; ++i) {
        float x = rs + (float)p * bin + ((float)i + .5f) * bin / (float)g;
        if (x <= 0.f) x = 0.f;
        int lo = (int)x, hi;
        if (lo >= n - 1) { hi = lo = n - 1; x = (float)lo; } else { hi = lo + 1; }
        const float l = x - (float)lo, h = 1.f - l;
        if (lo == at) w += h;
        if (hi == at) w += l;
    }
    return w;
}

#define ROIW_CT 8   // channels per thread

// d_feat[b, c, y, x] (= or +=) sum over the rays whose box reaches (y, x), in the fixed order of the source pixels
// (rows, then columns, then the pixel's list), of sum over bins of wy[ph] wx[pw] / count * d_out[r, (c S + ph) S + pw].
// A ray centred at (qx, qy) with corners u1 = clamp(qx - half) .. u2 = clamp(qx + half) taps columns u1 - 1 .. u2
// only, so the source pixels within half + 1 of (y, x) are all there is to visit.
__global__ void __launch_bounds__(256) lidf_roiw_gather_kernel(
    const float* __restrict__ d_out, long long ld, long long r0, const int* __restrict__ start,
    const int* __restrict__ list, int B, int Cn, int H, int W, int half, int S, int accumulate,
    float* __restrict__ d_feat) {
    const int ctiles = (Cn + ROIW_CT - 1) / ROIW_CT;
    const long long total = (long long)B * ctiles * H * W;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int x = (int)(i % W), y = (int)((i / W) % H);
    const long long bc = i / ((long long)W * H);
    const int ct = (int)(bc % ctiles);
    const long long b = bc / ctiles;
    const int c0 = ct * ROIW_CT;
    float acc[ROIW_CT];
#pragma unroll
    for (int j = 0; j < ROIW_CT; ++j) acc[j] = 0.f;
    const int ya = max(y - half - 1, 0), yb = min(y + half + 1, H - 1);
    const int xa = max(x - half - 1, 0), xb = min(x + half + 1, W - 1);
    for (int qy = ya; qy <= yb; ++qy) {
        const int v1 = min(max(qy - half, 0), H - 1), v2 = min(max(qy + half, 0), H - 1);
        if (y < v1 - 1 || y > v2) continue;
        const float rsh = (float)v1 - 0.5f, roi_h = ((float)v2 - 0.5f) - rsh;
        const float bin_h = roi_h / (float)S;
        const int gh = (int)ceilf(roi_h / (float)S);
        // the row weights depend on the source row alone: the first four bins' are kept over its pixels
        float wyc[4];
        bool any = S > 4;
#pragma unroll
        for (int ph = 0; ph < 4; ++ph) {
            wyc[ph] = ph < S ? roiw_axis_weight(rsh, bin_h, gh, ph, y, H) : 0.f;
            any = any || wyc[ph] != 0.f;
        }
        if (!any) continue;
        for (int qx = xa; qx <= xb; ++qx) {
            const size_t pix = ((size_t)b * H + qy) * W + qx;
            const int s0 = start[pix], s1 = start[pix + 1];
            if (s0 == s1) continue;
            const int u1 = min(max(qx - half, 0), W - 1), u2 = min(max(qx + half, 0), W - 1);
            if (x < u1 - 1 || x > u2) continue;
            const float rsw = (float)u1 - 0.5f, roi_w = ((float)u2 - 0.5f) - rsw;
            const float bin_w = roi_w / (float)S;
            const int gw = (int)ceilf(roi_w / (float)S);
            const float count = (float)max(gh * gw, 1);
            for (int pw = 0; pw < S; ++pw) {
                const float wx = roiw_axis_weight(rsw, bin_w, gw, pw, x, W);
                if (wx == 0.f) continue;
                const auto add = [&](int ph, float wy) {
                    const float wgt = wy * wx / count;
                    for (int s = s0; s < s1; ++s) {
                        const float* g = d_out + (size_t)(r0 + list[s]) * ld + ((size_t)c0 * S + ph) * S + pw;
#pragma unroll
                        for (int j = 0; j < ROIW_CT; ++j)
                            if (c0 + j < Cn) acc[j] += wgt * g[(size_t)j * S * S];
                    }
                };
#pragma unroll
                for (int ph = 0; ph < 4; ++ph)
                    if (wyc[ph] != 0.f) add(ph, wyc[ph]);
                for (int ph = 4; ph < S; ++ph) {
                    const float wy = roiw_axis_weight(rsh, bin_h, gh, ph, y, H);
                    if (wy != 0.f) add(ph, wy);
                }
            }
        }
    }
#pragma unroll
    for (int j = 0; j < ROIW_CT; ++j) {
        if (c0 + j >= Cn) break;
        float* dst = d_feat + (((size_t)b * Cn + c0 + j) * H + y) * W + x;
        *dst = accumulate ? *dst + acc[j] : acc[j];
    }
}

struct RoiwPlan {
    long long npix;
    size_t cnt, start, sums, list, total;
};
static RoiwPlan roiw_plan(long long B, long long H, long long W) {
    RoiwPlan p;
    p.npix = B * H * W;
    auto up = [](size_t x) { return (x + 255) / 256 * 256; };
    size_t o = 0;
    p.cnt = o;   o += up((size_t)p.npix * 4);
    p.start = o; o += up((size_t)(p.npix + 1) * 4);
    p.sums = o;  o += up((size_t)(p.npix / 1024 + 2) * 4);
    p.list = o;  o += up((size_t)p.npix * 4);     // one chunk of rays: as many as there are pixels
    p.total = o;
    return p;
}
extern "C" size_t lidf_roi_align_backward_ws_bytes(long long B, long long H, long long W) {
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    return roiw_plan(B, H, W).total;
}

// The rays go through in chunks of B H W (the list's capacity; every caller in pipeline.py has fewer rays than
// pixels: one chunk). The first chunk writes every element of d_feat, the later ones add to it, in order.
extern "C" hipError_t lidf_launch_roi_align_backward(const float* d_out, long long ld, const int* ray_pix,
                                                     const int* ray_bid, long long R, int B, int Cn, int H, int W,
                                                     int half, int S, float* d_feat, void* ws, hipStream_t st) {
    const RoiwPlan p = roiw_plan(B, H, W);
    char* w = (char*)ws;
    int* cnt = (int*)(w + p.cnt);
    int* start = (int*)(w + p.start);
    int* list = (int*)(w + p.list);
    const long long total = p.npix * ((Cn + ROIW_CT - 1) / ROIW_CT);
    for (long long r0 = 0; r0 < R; r0 += p.npix) {
        const long long r1 = r0 + p.npix < R ? r0 + p.npix : R;
        hipError_t e = hipMemsetAsync(cnt, 0, (size_t)p.npix * 4, st);
        if (e != hipSuccess) return e;
        const unsigned rb = (unsigned)((r1 - r0 + 255) / 256);
        hipLaunchKernelGGL(lidf_roiw_count_kernel, dim3(rb), dim3(256), 0, st, ray_pix, ray_bid, r0, r1, B, H, W, cnt);
        e = lidf_launch_scan(cnt, p.npix, start, (int*)(w + p.sums), st);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(lidf_roiw_fill_kernel, dim3(rb), dim3(256), 0, st, ray_pix, ray_bid, r0, r1, B, H, W, cnt,
                           start, list);
        hipLaunchKernelGGL(lidf_roiw_gather_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, d_out,
                           ld, r0, start, list, B, Cn, H, W, half, S, r0 > 0 ? 1 : 0, d_feat);
    }
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------------------------
// Sums of the rows of S [n, F] by an int32 row index, F any multiple of 4
// ------------------------------------------------------------------------------------------------------------------
#define SEGW_CH 128   // sorted rows per chunk sum (lidf_train.hip's SEG_CH)

struct SegwPlan {
    long long max_chunks;
    size_t sort, cnt, first, sums2, partial, total;
};
static SegwPlan segw_plan(long long n, long long V, int F) {
    SegwPlan s;
    s.max_chunks = n / SEGW_CH + V + 1;
    auto up = [](size_t x) { return (x + 255) / 256 * 256; };
    size_t o = 0;
    s.sort = o;    o += up(lidf_sort_idx_ws_bytes(n, V));
    s.cnt = o;     o += up((size_t)(V + 1) * 4);
    s.first = o;   o += up((size_t)(V + 2) * 4);
    s.sums2 = o;   o += up((size_t)(V / 1024 + 2) * 4);
    s.partial = o; o += up((size_t)s.max_chunks * F * 4);
    s.total = o;
    return s;
}
// 0: no sorted form at this size (more than 16,384 destination rows: the sort's histogram lives in LDS)
extern "C" size_t lidf_seg_sum_idx_any_ws_bytes(long long n, long long V, int F) {
    if (V > 16384 || V <= 0 || n <= 0 || F <= 0) return 0;
    return segw_plan(n, V, F).total;
}

// chunks of every destination row, from the sort's scan (scanned[v * nblk] = first sorted position of index v,
// scanned[V * nblk] = the number of rows placed)
__global__ void lidf_segw_chunks_kernel(const int* __restrict__ scanned, int V, int nblk, int* __restrict__ cnt) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= V) return;
    const long long beg = scanned[(size_t)v * nblk], end = scanned[(size_t)(v + 1) * nblk];
    cnt[v] = (int)((end - beg + SEGW_CH - 1) / SEGW_CH);
}

// partial[c, :] = the sum of chunk c's sorted rows: 4 row lanes x 64 column lanes of 4 floats, 256 columns a round;
// a row lane adds its rows in order, the four lanes are added in order.
__global__ void __launch_bounds__(256) lidf_segw_chunk_sum_kernel(
    const float* __restrict__ S, int F, const int* __restrict__ perm, const int* __restrict__ scanned,
    const int* __restrict__ first, int V, int nblk, float* __restrict__ partial) {
    __shared__ f32x4 red[4][64];
    const int c = blockIdx.x;
    if (c >= first[V]) return;
    int lo = 0, hi = V - 1;   // last index with first[v] <= c (indices without rows share their successor's value)
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (first[mid] <= c) lo = mid; else hi = mid - 1;
    }
    const int v = lo;
    const long long beg = (long long)scanned[(size_t)v * nblk] + (long long)(c - first[v]) * SEGW_CH;
    long long end = scanned[(size_t)(v + 1) * nblk];
    if (end > beg + SEGW_CH) end = beg + SEGW_CH;
    const int rl = threadIdx.x >> 6, c4 = threadIdx.x & 63;
    for (int j0 = 0; j0 < F; j0 += 256) {
        const int col = j0 + 4 * c4;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        if (col < F)
            for (long long i = beg + rl; i < end; i += 4) acc += *(const f32x4*)(S + (size_t)perm[i] * F + col);
        red[rl][c4] = acc;
        __syncthreads();
        if (rl == 0 && col < F) {
            f32x4 s = red[0][c4];
#pragma unroll
            for (int k = 1; k < 4; ++k) s += red[k][c4];
            *(f32x4*)(partial + (size_t)c * F + col) = s;
        }
        __syncthreads();
    }
}

// out[v, :] = the chunk sums of v added in chunk order (zero for an index without rows)
__global__ void __launch_bounds__(64) lidf_segw_final_kernel(const float* __restrict__ partial, int F,
                                                             const int* __restrict__ first,
                                                             float* __restrict__ out) {
    const int v = blockIdx.x;
    const int c0 = first[v], c1 = first[v + 1];
    for (int col = 4 * threadIdx.x; col < F; col += 256) {
        f32x4 s = {0.f, 0.f, 0.f, 0.f};
        for (int c = c0; c < c1; ++c) s += *(const f32x4*)(partial + (size_t)c * F + col);
        *(f32x4*)(out + (size_t)v * F + col) = s;
    }
}

// Above 16,384 destination rows: out (zeroed by the launcher) += S[p, :] with float atomics — a wavefront walks 64
// consecutive rows and flushes its running sum whenever the index changes (lidf_seg_sum_idx_kernel at any width;
// the summation order is not fixed).
__global__ void __launch_bounds__(256) lidf_segw_atomic_kernel(const float* __restrict__ S, int F,
                                                               const int* __restrict__ idx, long long n,
                                                               long long V, float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const long long p0 = ((long long)blockIdx.x * 4 + (threadIdx.x >> 6)) * 64;
    if (p0 >= n) return;
    const long long p1 = p0 + 64 < n ? p0 + 64 : n;
    for (int col = 4 * lane; col < F; col += 256) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        int cur = -1;
        for (long long p = p0; p <= p1; ++p) {
            int v = p < p1 ? idx[p] : -1;
            if (v < 0 || v >= V) v = -1;
            if (v != cur) {
                if (cur >= 0) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) atomicAdd(out + (size_t)cur * F + col + i, acc[i]);
                }
                acc = f32x4{0.f, 0.f, 0.f, 0.f};
                cur = v;
            }
            if (v >= 0) acc += *(const f32x4*)(S + (size_t)p * F + col);
        }
    }
}

// out[v, :] = sum of S[p, :] over the rows with idx[p] == v, for v < V (F % 4 == 0; rows whose index lies outside
// [0, V) are left out). With ws (lidf_seg_sum_idx_any_ws_bytes(n, V, F) > 0 bytes): the sorted form, no float atomics,
// rows added in row order within chunks of SEGW_CH and chunks in order. Without: zero + atomics.
extern "C" hipError_t lidf_launch_seg_sum_idx_any(const float* S, int F, const int* idx, long long n, long long V,
                                                  float* out, void* ws, size_t ws_bytes, hipStream_t st) {
    if (V <= 0) return hipSuccess;
    const size_t need = lidf_seg_sum_idx_any_ws_bytes(n, V, F);
    if (n <= 0 || need == 0 || !ws || ws_bytes < need) {
        hipError_t e = hipMemsetAsync(out, 0, (size_t)V * F * 4, st);
        if (e != hipSuccess || n <= 0) return e;
        hipLaunchKernelGGL(lidf_segw_atomic_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, S, F, idx, n,
                           V, out);
        return hipGetLastError();
    }
    const SegwPlan s = segw_plan(n, V, F);
    char* w = (char*)ws;
    const int *perm = nullptr, *n_perm = nullptr;
    hipError_t e = lidf_launch_sort_idx(idx, n, nullptr, V, w + s.sort, &perm, &n_perm, st);
    if (e != hipSuccess) return e;
    size_t scanned_off = 0, perm_off = 0;
    int nblk = 0;
    lidf_sort_idx_layout(n, V, &scanned_off, &nblk, &perm_off);
    const int* scanned = (const int*)(w + s.sort + scanned_off);
    int* cnt = (int*)(w + s.cnt);
    int* first = (int*)(w + s.first);
    float* partial = (float*)(w + s.partial);
    hipLaunchKernelGGL(lidf_segw_chunks_kernel, dim3((unsigned)((V + 255) / 256)), dim3(256), 0, st, scanned, (int)V,
                       nblk, cnt);
    e = lidf_launch_scan(cnt, V, first, (int*)(w + s.sums2), st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(lidf_segw_chunk_sum_kernel, dim3((unsigned)s.max_chunks), dim3(256), 0, st, S, F, perm, scanned,
                       first, (int)V, nblk, partial);
    hipLaunchKernelGGL(lidf_segw_final_kernel, dim3((unsigned)V), dim3(64), 0, st, partial, F, first, out);
    return hipGetLastError();
}
