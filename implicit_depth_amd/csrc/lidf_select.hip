// lidf_select.hip — hard-negative mining on the device: the mean of the k largest of n float32 values and the
// backward's weights (1/k at the selected elements), torch.topk + mean of models/pipeline.py:475-490, 514-539,
// 767-770, as a most-significant-digit radix select (11 + 11 + 10 bits of an order-preserving key):
//   lidf_select_hist_kernel<0|1|2>  per slab of 4096 values: the histogram of one digit in LDS, its non-empty bins
//                                   added to the job's global histogram (integer atomics: order-free). Rounds 1 and 2
//                                   re-derive the earlier rounds' buckets from the finished histograms themselves
//   lidf_select_partial_kernel      per slab: the number of values equal to the k-th value T and the double sum of
//                                   the values above it
//   lidf_select_final_kernel        one workgroup, job after job: the ties' prefix over the slabs in slab order, the
//                                   partial sums in a fixed order, mean = (sum + ties taken * T) / k; then loss_net of
//                                   the stage wrappers from the means (SelectCompose)
//   lidf_select_weights_kernel      per slab: 1/k above T and at the first (k - count above T) ties, ranked by the
//                                   slab prefix plus an ordered count inside the workgroup; 0 elsewhere
// Order: NaN > +inf > ... > -inf, -0.0 == +0.0, every NaN equal. Ties at the k-th value: the lowest indices win.
// k = (long long)((double)count * ratio) with count = n or a device int32 — computed on the device by every
// workgroup, so nothing is read back. Workgroups exchange data across launch boundaries only. The launch sequence
// depends on the jobs' sizes alone; the histograms are zeroed inside it, so a graph replay starts clean. No float
// atomics: the mean is bit-identical from run to run.
#include "lidf_launch.h"

#include <string.h>

namespace {

constexpr int SEL_BLOCK = 256;
constexpr int SEL_ITERS = 4;                           // float4 loads per thread and slab
constexpr int SEL_SLAB = SEL_BLOCK * SEL_ITERS * 4;    // 4096 values
constexpr int SEL_NB0 = 2048, SEL_NB1 = 2048, SEL_NB2 = 1024;   // bins of the digits: key >> 21, >> 10 & 2047, & 1023
constexpr int SEL_HIST = SEL_NB0 + SEL_NB1 + SEL_NB2;
constexpr int SEL_STATE = 4;                           // T, ties taken, k, unused

// A job as the kernels see it. Values are addressed by the "virtual" index v = i + off with off = the distance of
// values[0] from the 16-byte boundary below it (0..3 floats): vbase = values - off is 16-byte aligned, the job's
// elements are v in [off, off + n), slab s is v in [s * 4096, (s + 1) * 4096). The order of v is the order of i.
struct SelJob {
    const float* vbase;
    float* wbase;          // weights - off, or NULL
    long long lo, hi;      // off, off + n
    long long n;
    const int* count;
    float* mean;
    unsigned* hist;        // [SEL_HIST]
    unsigned* state;       // [SEL_STATE]
    unsigned* tie_cnt;     // [nslab]
    unsigned* tie_pre;     // [nslab]
    double* partial;       // [nslab]
    int nslab;
    int w_vec;             // wbase is 16-byte aligned
};

struct SelJobs {
    SelJob j[LIDF_SELECT_MAX_JOBS];
    int n_jobs;
    double ratio;
};

// Larger key = greater value in torch.topk's order.
__device__ __forceinline__ unsigned sel_key(float v) {
    if (v != v) return 0xffffffffu;
    unsigned b = __float_as_uint(v);
    if (b == 0x80000000u) b = 0u;
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__device__ __forceinline__ float sel_value(unsigned key) {
    if (key == 0xffffffffu) return __uint_as_float(0x7fc00000u);
    return __uint_as_float((key & 0x80000000u) ? (key & 0x7fffffffu) : ~key);
}

__device__ __forceinline__ long long sel_k(const SelJob& j, double ratio) {
    long long cnt = j.count ? (long long)*j.count : j.n;
    cnt = cnt < 0 ? 0 : (cnt > j.n ? j.n : cnt);
    const long long k = (long long)((double)cnt * ratio);
    return k < 0 ? 0 : (k > j.n ? j.n : k);
}

// Four consecutive values at virtual index 4q: one 16-byte load when they all belong to the job.
__device__ __forceinline__ void sel_load(const SelJob& j, long long q, float* v, bool* ok) {
    const long long v0 = 4 * q;
    if (v0 >= j.lo && v0 + 4 <= j.hi) {
        const f32x4 x = *reinterpret_cast<const f32x4*>(j.vbase + v0);
        v[0] = x[0], v[1] = x[1], v[2] = x[2], v[3] = x[3];
        ok[0] = ok[1] = ok[2] = ok[3] = true;
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            ok[i] = v0 + i >= j.lo && v0 + i < j.hi;
            v[i] = ok[i] ? j.vbase[v0 + i] : 0.f;
        }
    }
}

// The bin that holds the k-th largest element of a finished histogram (1 <= k <= its total) and how many are still
// to take inside it. Thread t owns bins NB-1 - (t*PER .. t*PER+PER-1), the highest first. sh: 6 words.
struct SelPick {
    unsigned bin, krem;
};

template <int NB>
__device__ __forceinline__ SelPick sel_pick(const unsigned* __restrict__ hist, unsigned k, unsigned* sh) {
    constexpr int PER = NB / SEL_BLOCK;
    const int t = threadIdx.x;
    unsigned c[PER], s = 0;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        c[i] = hist[NB - 1 - (t * PER + i)];
        s += c[i];
    }
    if (t == 0) sh[4] = 0u, sh[5] = 1u;
    unsigned total;
    unsigned cum = block_scan<SEL_BLOCK>(s, sh, total);   // (its first barrier also orders the two stores above)
    if (cum < k && k <= cum + s) {
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            if (cum < k && k <= cum + c[i]) sh[4] = (unsigned)(NB - 1 - (t * PER + i)), sh[5] = k - cum;
            cum += c[i];
        }
    }
    __syncthreads();
    SelPick p;
    p.bin = sh[4], p.krem = sh[5];
    __syncthreads();
    return p;
}

// The k-th largest key T (k >= 1) and the number of elements equal to T that are selected.
__device__ __forceinline__ unsigned sel_threshold(const SelJob& j, unsigned k, unsigned* sh, unsigned& ktie) {
    const SelPick p0 = sel_pick<SEL_NB0>(j.hist, k, sh);
    const SelPick p1 = sel_pick<SEL_NB1>(j.hist + SEL_NB0, p0.krem, sh);
    const SelPick p2 = sel_pick<SEL_NB2>(j.hist + SEL_NB0 + SEL_NB1, p1.krem, sh);
    ktie = p2.krem;
    return (p0.bin << 21) | (p1.bin << 10) | p2.bin;
}

template <int ROUND>
__global__ __launch_bounds__(SEL_BLOCK) void lidf_select_hist_kernel(const SelJobs J) {
    const SelJob& j = J.j[blockIdx.y];
    if ((int)blockIdx.x >= j.nslab) return;
    __shared__ unsigned lh[SEL_NB0];
    __shared__ unsigned sh[8];
    constexpr int NB = ROUND == 2 ? SEL_NB2 : SEL_NB0;
    const long long k = sel_k(j, J.ratio);
    if (k == 0) return;
    unsigned prefix = 0;   // the digits above this round's
    if constexpr (ROUND >= 1) {
        const SelPick p0 = sel_pick<SEL_NB0>(j.hist, (unsigned)k, sh);
        prefix = p0.bin;
        if constexpr (ROUND == 2) {
            const SelPick p1 = sel_pick<SEL_NB1>(j.hist + SEL_NB0, p0.krem, sh);
            prefix = (prefix << 11) | p1.bin;
        }
    }
    for (int b = threadIdx.x; b < NB; b += SEL_BLOCK) lh[b] = 0u;
    __syncthreads();
#pragma unroll
    for (int it = 0; it < SEL_ITERS; ++it) {
        const long long q = ((long long)blockIdx.x * SEL_ITERS + it) * SEL_BLOCK + threadIdx.x;
        float v[4];
        bool ok[4];
        sel_load(j, q, v, ok);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const unsigned key = sel_key(v[i]);
            bool in = ok[i];
            unsigned d;
            if constexpr (ROUND == 0) d = key >> 21;
            if constexpr (ROUND == 1) d = (key >> 10) & 2047u, in = in && (key >> 21) == prefix;
            if constexpr (ROUND == 2) d = key & 1023u, in = in && (key >> 10) == prefix;
            if (in) atomicAdd(&lh[d], 1u);
        }
    }
    __syncthreads();
    unsigned* g = j.hist + (ROUND == 0 ? 0 : (ROUND == 1 ? SEL_NB0 : SEL_NB0 + SEL_NB1));
    for (int b = threadIdx.x; b < NB; b += SEL_BLOCK) {
        const unsigned c = lh[b];
        if (c) atomicAdd(&g[b], c);
    }
}

// The workgroup's sum in a fixed order: wavefront butterflies, then the four wavefronts in order (thread 0 holds it).
__device__ __forceinline__ double sel_block_sum(double v, double* dsh) {
    const double t = wave_sum(v);
    if ((threadIdx.x & 63) == 0) dsh[threadIdx.x >> 6] = t;
    __syncthreads();
    double r = 0.0;
#pragma unroll
    for (int w = 0; w < SEL_BLOCK / 64; ++w) r += dsh[w];
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(SEL_BLOCK) void lidf_select_partial_kernel(const SelJobs J) {
    const SelJob& j = J.j[blockIdx.y];
    if ((int)blockIdx.x >= j.nslab) return;
    __shared__ unsigned sh[8];
    __shared__ double dsh[SEL_BLOCK / 64];
    const long long k = sel_k(j, J.ratio);
    if (k == 0) return;   // (the final kernel reads neither array then)
    unsigned ktie;
    const unsigned T = sel_threshold(j, (unsigned)k, sh, ktie);
    double acc = 0.0;
    unsigned eq = 0;
#pragma unroll
    for (int it = 0; it < SEL_ITERS; ++it) {
        const long long q = ((long long)blockIdx.x * SEL_ITERS + it) * SEL_BLOCK + threadIdx.x;
        float v[4];
        bool ok[4];
        sel_load(j, q, v, ok);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const unsigned key = sel_key(v[i]);
            if (ok[i] && key > T) acc += (double)v[i];
            eq += (ok[i] && key == T) ? 1u : 0u;
        }
    }
    unsigned eq_total;
    block_scan<SEL_BLOCK>(eq, sh, eq_total);
    const double sum = sel_block_sum(acc, dsh);
    if (threadIdx.x == 0) j.tie_cnt[blockIdx.x] = eq_total, j.partial[blockIdx.x] = sum;
}

__global__ __launch_bounds__(SEL_BLOCK) void lidf_select_final_kernel(const SelJobs J, const SelectCompose Cm) {
    __shared__ unsigned sh[8];
    __shared__ double dsh[SEL_BLOCK / 64];
    __shared__ float means[LIDF_SELECT_MAX_JOBS];
    for (int jj = 0; jj < J.n_jobs; ++jj) {
        const SelJob& j = J.j[jj];
        const long long k = j.n > 0 ? sel_k(j, J.ratio) : 0;
        unsigned T = 0, ktie = 0;
        double total = 0.0;
        if (k > 0) {
            T = sel_threshold(j, (unsigned)k, sh, ktie);
            unsigned carry = 0;
            for (int base = 0; base < j.nslab; base += SEL_BLOCK) {
                const int s = base + threadIdx.x;
                const unsigned c = s < j.nslab ? j.tie_cnt[s] : 0u;
                unsigned tot;
                const unsigned exc = block_scan<SEL_BLOCK>(c, sh, tot);
                if (s < j.nslab) j.tie_pre[s] = carry + exc;
                carry += tot;
            }
            double acc = 0.0;
            for (int s = threadIdx.x; s < j.nslab; s += SEL_BLOCK) acc += j.partial[s];
            total = sel_block_sum(acc, dsh);
        }
        if (threadIdx.x == 0) {
            if (k > 0) total += (double)ktie * (double)sel_value(T);
            const float m = (float)(total / (double)k);   // k == 0: 0 / 0 = NaN, torch.mean of an empty tensor
            means[jj] = m;
            if (j.mean) *j.mean = m;
            j.state[0] = T, j.state[1] = ktie, j.state[2] = (unsigned)k;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0 && Cm.mode != 0) {
        // the order of lidf_loss_final_kernel
        const float pos = means[0], surf = means[1], smooth = means[2] + means[3];
        float net = Cm.pos_w * pos;
        if (Cm.mode == 1) net = net + Cm.prob_w * means[4];
        if (Cm.surf_on) net += Cm.surf_w * surf;
        if (Cm.smooth_on) net += Cm.smooth_w * smooth;
        if (Cm.mode == 1) {
            Cm.loss[0] = pos, Cm.loss[1] = means[4], Cm.loss[2] = surf, Cm.loss[3] = smooth, Cm.loss[4] = net;
        } else {
            Cm.loss[0] = pos, Cm.loss[1] = surf, Cm.loss[2] = smooth, Cm.loss[3] = net;
        }
    }
}

__global__ __launch_bounds__(SEL_BLOCK) void lidf_select_weights_kernel(const SelJobs J) {
    const SelJob& j = J.j[blockIdx.y];
    if ((int)blockIdx.x >= j.nslab || !j.wbase) return;
    __shared__ unsigned sh[8];
    const unsigned T = j.state[0], ktie = j.state[1], k = j.state[2];
    const float w = k ? (float)(1.0 / (double)k) : 0.f;
    // the slab's ties: all taken, none taken, or ranked in index order (the boundary slab only)
    unsigned run = 0, tcnt = 0;
    if (k) run = j.tie_pre[blockIdx.x], tcnt = j.tie_cnt[blockIdx.x];
    const bool none = k == 0 || run >= ktie;
    const bool all = !none && run + tcnt <= ktie;
    const bool ranked = !none && !all;
#pragma unroll
    for (int it = 0; it < SEL_ITERS; ++it) {
        const long long q = ((long long)blockIdx.x * SEL_ITERS + it) * SEL_BLOCK + threadIdx.x;
        float v[4], o[4];
        bool ok[4], eq[4];
        sel_load(j, q, v, ok);
        unsigned c = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const unsigned key = sel_key(v[i]);
            eq[i] = ok[i] && k != 0 && key == T;
            o[i] = (k != 0 && key > T) || (eq[i] && all) ? w : 0.f;
            c += eq[i] ? 1u : 0u;
        }
        if (ranked) {   // (the same in every thread of the workgroup)
            unsigned tot;
            unsigned r = run + block_scan<SEL_BLOCK>(c, sh, tot);
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (eq[i]) {
                    o[i] = r < ktie ? w : 0.f;
                    ++r;
                }
            run += tot;
        }
        const long long v0 = 4 * q;
        if (j.w_vec && ok[0] && ok[3]) {
            f32x4 x;
            x[0] = o[0], x[1] = o[1], x[2] = o[2], x[3] = o[3];
            *reinterpret_cast<f32x4*>(j.wbase + v0) = x;
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (ok[i]) j.wbase[v0 + i] = o[i];
        }
    }
}

inline size_t sel_align(size_t b) { return (b + 255) & ~(size_t)255; }
inline long long sel_slabs(long long n) { return n > 0 ? (n + 3 + SEL_SLAB - 1) / SEL_SLAB : 0; }   // (off <= 3)

}  // namespace

// [histograms of every job | states | per job: partial sums | per job: tie counts, tie prefixes]
extern "C" size_t lidf_select_workspace_bytes(int n_jobs, long long n_max) {
    if (n_jobs < 1 || n_jobs > LIDF_SELECT_MAX_JOBS || n_max < 0) return 0;
    const size_t slabs = (size_t)sel_slabs(n_max);
    return sel_align((size_t)n_jobs * SEL_HIST * sizeof(unsigned)) +
           sel_align((size_t)n_jobs * SEL_STATE * sizeof(unsigned)) +
           (size_t)n_jobs * (sel_align(slabs * sizeof(double)) + 2 * sel_align(slabs * sizeof(unsigned)));
}

extern "C" hipError_t lidf_launch_select(const SelectJob* jobs, int n_jobs, double ratio, const SelectCompose& c,
                                         void* ws, hipStream_t st) {
    long long n_max = 0;
    for (int i = 0; i < n_jobs; ++i) n_max = jobs[i].n > n_max ? jobs[i].n : n_max;
    const size_t slabs = (size_t)sel_slabs(n_max);
    const size_t hist_bytes = sel_align((size_t)n_jobs * SEL_HIST * sizeof(unsigned));
    char* p = (char*)ws;
    unsigned* hist = (unsigned*)p;
    p += hist_bytes;
    unsigned* state = (unsigned*)p;
    p += sel_align((size_t)n_jobs * SEL_STATE * sizeof(unsigned));
    SelJobs J;
    memset(&J, 0, sizeof(J));
    J.n_jobs = n_jobs, J.ratio = ratio;
    int grid_x = 0;
    bool any_w = false;
    for (int i = 0; i < n_jobs; ++i) {
        SelJob& j = J.j[i];
        const SelectJob& s = jobs[i];
        const long long off = s.n > 0 ? (long long)(((uintptr_t)s.values & 15) >> 2) : 0;
        j.vbase = s.n > 0 ? s.values - off : nullptr;
        j.wbase = (s.n > 0 && s.weights) ? s.weights - off : nullptr;
        j.w_vec = j.wbase && ((uintptr_t)j.wbase & 15) == 0;
        j.lo = off, j.hi = off + s.n, j.n = s.n;
        j.count = s.count, j.mean = s.mean;
        j.hist = hist + (size_t)i * SEL_HIST, j.state = state + (size_t)i * SEL_STATE;
        j.partial = (double*)p;
        p += sel_align(slabs * sizeof(double));
        j.tie_cnt = (unsigned*)p;
        p += sel_align(slabs * sizeof(unsigned));
        j.tie_pre = (unsigned*)p;
        p += sel_align(slabs * sizeof(unsigned));
        j.nslab = s.n > 0 ? (int)((off + s.n + SEL_SLAB - 1) / SEL_SLAB) : 0;
        grid_x = j.nslab > grid_x ? j.nslab : grid_x;
        any_w = any_w || j.wbase;
    }
    if (grid_x > 0) {
        hipError_t e = hipMemsetAsync(hist, 0, hist_bytes, st);
        if (e != hipSuccess) return e;
        const dim3 grid((unsigned)grid_x, (unsigned)n_jobs), block(SEL_BLOCK);
        hipLaunchKernelGGL(lidf_select_hist_kernel<0>, grid, block, 0, st, J);
        hipLaunchKernelGGL(lidf_select_hist_kernel<1>, grid, block, 0, st, J);
        hipLaunchKernelGGL(lidf_select_hist_kernel<2>, grid, block, 0, st, J);
        hipLaunchKernelGGL(lidf_select_partial_kernel, grid, block, 0, st, J);
    }
    hipLaunchKernelGGL(lidf_select_final_kernel, dim3(1), dim3(SEL_BLOCK), 0, st, J, c);
    if (grid_x > 0 && any_w)
        hipLaunchKernelGGL(lidf_select_weights_kernel, dim3((unsigned)grid_x, (unsigned)n_jobs), dim3(SEL_BLOCK), 0,
                           st, J);
    return hipGetLastError();
}
