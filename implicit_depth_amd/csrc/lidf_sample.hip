// lidf_sample.hip — the random block sampler of the valid points: utils/point_utils.py:79-125
// sample_valid_points (what LIDF.get_valid_points keeps when grid.valid_sample_num != -1,
// models/pipeline.py:137-160), on the device and without a size read.
//
// "Block order" is the reference's: 8x8 blocks in row-major order, pixels in row-major order inside a
// block. One wave is one block: __ballot over the 64 pixels is the block's occupancy mask, its popcount
// the block's number of valid pixels. Three small launches on the caller's stream:
//   1  masks[blk] = ballot of block blk, the whole batch in one grid   (the only read of the mask: h*w elements
//                                                                       per image)
//   2  prefix[blk] = number of valid pixels in blocks < blk: one workgroup per image, chunks of SAMPLE_THREADS
//      blocks with a carry; prefix[nblk] = valid_cnt
//   3  slot i -> block-order rank -> pixel, one thread per slot: a binary search over prefix, then the k-th set bit
//      of one mask
// masks and prefix live in the caller's workspace (any block count; LDS does not grow with the image).
// No compacted pixel list exists at any point. (All three as phases of ONE launch with one workgroup per image
// was the first version: 73 us at 240 x 320, n = 10000 — ten slots per thread, each an 11-step dependent search —
// against the launches below)
//
// Per image, cnt valid pixels, n = sample_num (semantics of point_utils.py:99-116):
//   dense  (cnt >= n): step = cnt / n, inum = cnt / step; slot i takes interval j_i = perm(i), perm a keyed
//          bijection of [0, inum), and rank j_i * step + off_i with off_i uniform in [0, step)
//   sparse (0 < cnt < n): slots 0 .. cnt-1 are every valid point in block order; slot i >= cnt takes pool entry
//          q = perm(i - cnt), perm a keyed bijection of [0, M), M = (ceil(n / cnt) - 1) * cnt, rank q mod cnt
//   empty  (cnt == 0): (b, 0) in every slot, valid_cnt[b] = 0 (the reference's assertion; the callers that
//          read sizes raise)
// Randomness is counter-based and integer-only: Philox4x32-10 keyed by the 64-bit seed, counter words
// (call counter lo, hi, image, slot | purpose); both come from device memory (rng_state), so a captured
// graph draws fresh samples on every replay once the caller advances the counter. perm is a balanced
// Feistel network of SAMPLE_ROUNDS rounds on 2 * ceil(bits / 2) bits with cycle walking: evaluating it at
// 0 .. n-1 gives n distinct values in random order at O(1) per slot. Uniform integers are
// (u32 * range) >> 32. tests/sampler_ref.py restates all of it in numpy, bit for bit.
// The second half of the file is the other random draw of the training front end, the window of the miss rays
// (lidf_miss_ray_window_f32), on the same Philox and the same state.
#include "lidf_launch.h"

#define SAMPLE_THREADS 1024
#define SAMPLE_WAVES (SAMPLE_THREADS / 64)
#define SAMPLE_BLOCK_WAVES 4      // 8x8 blocks per workgroup of the ballot launch
#define SAMPLE_SLOT_THREADS 256   // slots per workgroup of the sampling launch
#define SAMPLE_ROUNDS 6
#define SAMPLE_KEY_WORD 0x80000000u   // counter word 3 of the per-image key draws (slots are < 2^31)

__device__ __forceinline__ void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0,
                                              unsigned k1, unsigned out[4]) {
    for (int r = 0; r < 10; ++r) {
        const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

__device__ __forceinline__ unsigned sample_mix(unsigned v) {
    v ^= v >> 16; v *= 0x7FEB352Du;
    v ^= v >> 15; v *= 0x846CA68Bu;
    v ^= v >> 16;
    return v;
}

// keyed bijection of [0, N): Feistel on 2h bits (2^(2h) < 4N for N > 1), walked until it lands below N
__device__ __forceinline__ unsigned sample_perm(unsigned x, unsigned N, int h, const unsigned* key) {
    const unsigned m = (1u << h) - 1u;
    do {
        unsigned L = x >> h, R = x & m;
        for (int r = 0; r < SAMPLE_ROUNDS; ++r) {
            const unsigned t = L ^ (sample_mix(R + key[r]) & m);
            L = R;
            R = t;
        }
        x = (L << h) | R;
    } while (x >= N);
    return x;
}

// position of the k-th (0-based) set bit of m; k < popcount(m)
__device__ __forceinline__ int sample_select_bit(unsigned long long m, int k) {
    int pos = 0;
    for (int wd = 32; wd >= 1; wd >>= 1) {
        const unsigned long long low = m & ((1ull << wd) - 1ull);
        const int c = __popcll(low);
        if (k >= c) {
            k -= c;
            pos += wd;
            m >>= wd;
        } else {
            m = low;
        }
    }
    return pos;
}

// 1: one wave, one 8x8 block; SAMPLE_BLOCK_WAVES blocks per workgroup, the whole batch in one grid
__global__ __launch_bounds__(64 * SAMPLE_BLOCK_WAVES) void lidf_sample_blocks_kernel(
    const void* __restrict__ mask, int dtype, int H, int W, unsigned long long* __restrict__ masks) {
    const int b = blockIdx.y, lane = threadIdx.x & 63;
    const int bw = W >> 3, nblk = (H >> 3) * bw;
    const int blk = blockIdx.x * SAMPLE_BLOCK_WAVES + (threadIdx.x >> 6);
    if (blk >= nblk) return;   // (uniform per wave)
    const int by = blk / bw, bx = blk - by * bw;
    const long long pix = (long long)b * H * W + (long long)(by * 8 + (lane >> 3)) * W + bx * 8 + (lane & 7);
    const unsigned long long m = __ballot(mask_nonzero(mask, dtype, pix));
    if (lane == 0) masks[(size_t)b * nblk + blk] = m;
}

// 2: exclusive scan of the block counts of one image per workgroup, in chunks of SAMPLE_THREADS blocks
__global__ __launch_bounds__(SAMPLE_THREADS) void lidf_sample_scan_kernel(
    const unsigned long long* __restrict__ masks, int nblk, int* __restrict__ prefix, int* __restrict__ valid_cnt) {
    __shared__ int s_wave[SAMPLE_WAVES];
    const int b = blockIdx.x, tid = threadIdx.x;
    const unsigned long long* mk = masks + (size_t)b * nblk;
    int* pre = prefix + (size_t)b * (nblk + 1);
    if (tid == 0) pre[0] = 0;
    int carry = 0;
    for (int base = 0; base < nblk; base += SAMPLE_THREADS) {
        const int blk = base + tid;
        const int c = blk < nblk ? __popcll(mk[blk]) : 0;
        int tot;
        const int ex = block_scan<SAMPLE_THREADS>(c, s_wave, tot);
        if (blk < nblk) pre[blk + 1] = carry + ex + c;
        carry += tot;
    }
    if (tid == 0) valid_cnt[b] = carry;
}

// 3: one thread, one slot
__global__ __launch_bounds__(SAMPLE_SLOT_THREADS) void lidf_sample_slots_kernel(
    int H, int W, int n, const unsigned long long* __restrict__ rng, int* __restrict__ bid, int* __restrict__ flat,
    long long* __restrict__ idx, const unsigned long long* __restrict__ masks, const int* __restrict__ prefix) {
    const int b = blockIdx.y, i = blockIdx.x * SAMPLE_SLOT_THREADS + threadIdx.x;
    if (i >= n) return;
    const int bw = W >> 3, nblk = (H >> 3) * bw;
    const unsigned long long* mk = masks + (size_t)b * nblk;
    const int* pre = prefix + (size_t)b * (nblk + 1);
    const int cnt = pre[nblk];
    const long long s = (long long)b * n + i;
    int f = 0;
    if (cnt > 0) {
        const unsigned long long seed = rng[0], ctr = rng[1];
        const unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32);
        const unsigned c0 = (unsigned)ctr, c1 = (unsigned)(ctr >> 32);
        const bool dense = cnt >= n;
        const unsigned step = dense ? (unsigned)(cnt / n) : 1u;
        const unsigned N = dense ? (unsigned)cnt / step : (unsigned)((n + cnt - 1) / cnt - 1) * (unsigned)cnt;
        const int bits = N > 1 ? 32 - __clz((int)(N - 1)) : 0;
        const int h = (bits + 1) >> 1;
        unsigned rank;
        if (dense || i >= cnt) {
            unsigned key[8];
            philox4x32_10(c0, c1, (unsigned)b, SAMPLE_KEY_WORD, k0, k1, key);
            philox4x32_10(c0, c1, (unsigned)b, SAMPLE_KEY_WORD + 1u, k0, k1, key + 4);
            if (dense) {
                const unsigned j = sample_perm((unsigned)i, N, h, key);
                unsigned off = 0;
                if (step > 1) {
                    unsigned r[4];
                    philox4x32_10(c0, c1, (unsigned)b, (unsigned)i, k0, k1, r);
                    off = __umulhi(r[0], step);
                }
                rank = j * step + off;
            } else {
                rank = sample_perm((unsigned)(i - cnt), N, h, key) % (unsigned)cnt;
            }
        } else {
            rank = (unsigned)i;
        }
        int lo = 0, hi = nblk;   // the block with prefix[blk] <= rank < prefix[blk + 1]
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if ((unsigned)pre[mid] <= rank) lo = mid; else hi = mid;
        }
        const int p = sample_select_bit(mk[lo], (int)rank - pre[lo]);
        const int by = lo / bw, bx = lo - by * bw;
        f = (by * 8 + (p >> 3)) * W + bx * 8 + (p & 7);
    }
    bid[s] = b;
    flat[s] = f;
    if (idx) {
        idx[2 * s] = b;
        idx[2 * s + 1] = f;
    }
}

extern "C" size_t lidf_sample_valid_masks_bytes(int B, int H, int W) {
    const size_t nblk = (size_t)(H / 8) * (size_t)(W / 8);
    return ((size_t)B * nblk * 8 + 255) / 256 * 256;
}

extern "C" size_t lidf_sample_valid_ws_bytes(int B, int H, int W) {
    const size_t nblk = (size_t)(H / 8) * (size_t)(W / 8);
    return lidf_sample_valid_masks_bytes(B, H, W) + ((size_t)B * (nblk + 1) * 4 + 255) / 256 * 256;
}

extern "C" hipError_t lidf_launch_sample_valid(const void* mask, int dtype, int B, int H, int W, int n,
                                               const unsigned long long* rng, int* bid, int* flat, long long* idx,
                                               int* valid_cnt, void* ws, hipStream_t st) {
    unsigned long long* masks = (unsigned long long*)ws;
    int* prefix = (int*)((char*)ws + lidf_sample_valid_masks_bytes(B, H, W));
    const int nblk = (H / 8) * (W / 8);
    hipLaunchKernelGGL(lidf_sample_blocks_kernel, dim3((unsigned)((nblk + SAMPLE_BLOCK_WAVES - 1) / SAMPLE_BLOCK_WAVES),
                                                       (unsigned)B),
                       dim3(64 * SAMPLE_BLOCK_WAVES), 0, st, mask, dtype, H, W, masks);
    hipLaunchKernelGGL(lidf_sample_scan_kernel, dim3((unsigned)B), dim3(SAMPLE_THREADS), 0, st, masks, nblk, prefix,
                       valid_cnt);
    hipLaunchKernelGGL(lidf_sample_slots_kernel, dim3((unsigned)((n + SAMPLE_SLOT_THREADS - 1) / SAMPLE_SLOT_THREADS),
                                                      (unsigned)B),
                       dim3(SAMPLE_SLOT_THREADS), 0, st, H, W, n, rng, bid, flat, idx, masks, prefix);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------------------------
// The random window of the miss rays: LIDF.get_miss_ray, models/pipeline.py:232-254 (what training keeps of the
// corrupt pixels when grid.miss_sample_num != -1), without compacting the pixels outside the windows and without a
// size read. Image b has cnt_b non-zero pixels, T = sum cnt_b, n = miss_sample_num:
//   sampling = B * n < T (strict, :232); sampling and cnt_b > n: the ranks [s_b, s_b + n) of the image's non-zero
//   pixels in ascending pixel order, s_b uniform in [0, cnt_b - n]; every other image keeps all cnt_b (s_b = 0).
// s_b = __umulhi(r[0], cnt_b - n + 1), r the Philox block of counter words (call counter lo, hi, b,
// SAMPLE_KEY_WORD + 2) — a domain the valid sampler above never draws from, so both share one state —, or
// clamp(starts[b], 0, cnt_b - n) when the caller passes starts. Three launches on the caller's stream:
//   1  block_cnt[blk] = non-zero pixels of every block of MISS_ITEMS pixels (lidf_miss_count_kernel, lidf_aux.hip)
//   2  ONE workgroup: block_off = exclusive scan of block_cnt; img_off[b] = non-zero pixels before image b, one wave
//      per image boundary: the offset of the boundary's block plus the pixels of the partial block in front of it
//      (h * w is no multiple of MISS_ITEMS in general); then one thread per image: the window (cnt, s, len, dst),
//      dst the exclusive scan of len, and n_rays = (sum len, T)
//   3  the fill pass of get_miss_ray with one more test: a non-zero pixel of global rank j is rank j - img_off[b] of
//      its image and is written — at dst_b + rank - s_b, so in (image, pixel) order without an atomic — only if that
//      lies in [s_b, s_b + len_b). No list of all T pixels exists at any point; rows >= sum len are not written.
// tests/miss_window_ref.py restates the selection in numpy, bit for bit.
__global__ __launch_bounds__(SAMPLE_THREADS) void lidf_miss_window_kernel(
    const void* __restrict__ mask, int dtype, int B, long long hw, int n, const unsigned long long* __restrict__ rng,
    const int* __restrict__ starts, const int* __restrict__ block_cnt, long long nb, int* block_off, int* img_off,
    int* __restrict__ window, int* __restrict__ n_rays) {
    __shared__ int s_wave[SAMPLE_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int T = 0;
    for (long long base = 0; base < nb; base += SAMPLE_THREADS) {
        const long long blk = base + tid;
        const int c = blk < nb ? block_cnt[blk] : 0;
        int tot;
        const int ex = block_scan<SAMPLE_THREADS>(c, s_wave, tot);
        if (blk < nb) block_off[blk] = T + ex;
        T += tot;
    }
    __syncthreads();   // (block_off is read below by other threads of this workgroup)
    for (int b = wave; b <= B; b += SAMPLE_WAVES) {
        const long long p = (long long)b * hw, blk = p / MISS_ITEMS;
        int v = 0;
        for (long long i = blk * MISS_ITEMS + lane; i < p; i += 64) v += mask_nonzero(mask, dtype, i) ? 1 : 0;
        v = wave_sum(v);
        if (lane == 0) img_off[b] = (blk < nb ? block_off[blk] : T) + v;
    }
    __syncthreads();   // (img_off likewise)
    const bool sampling = (long long)B * n < (long long)T;
    unsigned k0 = 0, k1 = 0, c0 = 0, c1 = 0;
    if (!starts) {
        const unsigned long long seed = rng[0], ctr = rng[1];
        k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32);
        c0 = (unsigned)ctr, c1 = (unsigned)(ctr >> 32);
    }
    int run = 0;
    for (int base = 0; base < B; base += SAMPLE_THREADS) {
        const int b = base + tid;
        int cnt = 0, s = 0, len = 0;
        if (b < B) {
            cnt = img_off[b + 1] - img_off[b];
            len = cnt;
            if (sampling && cnt > n) {
                len = n;
                if (starts) {
                    s = min(max(starts[b], 0), cnt - n);
                } else {
                    unsigned r[4];
                    philox4x32_10(c0, c1, (unsigned)b, SAMPLE_KEY_WORD + 2u, k0, k1, r);
                    s = (int)__umulhi(r[0], (unsigned)(cnt - n + 1));
                }
            }
        }
        int tot;
        const int dst = run + block_scan<SAMPLE_THREADS>(len, s_wave, tot);
        if (b < B) {
            window[4 * b] = cnt;
            window[4 * b + 1] = s;
            window[4 * b + 2] = len;
            window[4 * b + 3] = dst;
        }
        run += tot;
    }
    if (tid == 0) {
        n_rays[0] = run;
        n_rays[1] = T;
    }
}

__global__ __launch_bounds__(256) void lidf_miss_window_fill_kernel(
    const void* __restrict__ mask, int dtype, long long npix, const int* __restrict__ block_off,
    const int* __restrict__ img_off, const int* __restrict__ window, const float* __restrict__ intr, int H, int W,
    int* __restrict__ ray_bid, int* __restrict__ ray_flat, int* __restrict__ ray_pix, float* __restrict__ ray_dir,
    long long* __restrict__ bid64, long long* __restrict__ flat64, long long* __restrict__ pix64) {
    __shared__ int s_tmp[4];
    const long long b0 = (long long)blockIdx.x * MISS_ITEMS + threadIdx.x * 4;
    bool f[4];
    int v = 0;
    for (int k = 0; k < 4; ++k) {
        f[k] = b0 + k < npix && mask_nonzero(mask, dtype, b0 + k);
        v += f[k] ? 1 : 0;
    }
    int total;
    int j = block_off[blockIdx.x] + block_scan<256>(v, s_tmp, total);
    const long long hw = (long long)H * W;
    for (int k = 0; k < 4; ++k) {
        if (!f[k]) continue;
        const long long i = b0 + k;
        const int b = (int)(i / hw);
        const int rank = j - img_off[b];
        const int s = window[4 * b + 1], len = window[4 * b + 2];
        if (rank >= s && rank - s < len)
            miss_ray_write((long long)window[4 * b + 3] + (rank - s), b, (int)(i % hw), W, intr, ray_bid, ray_flat,
                           ray_pix, ray_dir, bid64, flat64, pix64);
        ++j;
    }
}

extern "C" hipError_t lidf_launch_miss_window(const void* mask, int dtype, const float* intr, int B, int H, int W,
                                              int n, const unsigned long long* rng, const int* starts, int* block_cnt,
                                              int* block_off, int* img_off, int* ray_bid, int* ray_flat, int* ray_pix,
                                              float* ray_dir, long long* bid64, long long* flat64, long long* pix64,
                                              int* window, int* n_rays, hipStream_t st) {
    const long long hw = (long long)H * W, npix = (long long)B * hw;
    const long long nb = (npix + MISS_ITEMS - 1) / MISS_ITEMS;
    hipError_t e = lidf_launch_miss_block_count(mask, dtype, npix, block_cnt, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(lidf_miss_window_kernel, dim3(1), dim3(SAMPLE_THREADS), 0, st, mask, dtype, B, hw, n, rng,
                       starts, (const int*)block_cnt, nb, block_off, img_off, window, n_rays);
    hipLaunchKernelGGL(lidf_miss_window_fill_kernel, dim3((unsigned)nb), dim3(256), 0, st, mask, dtype, npix,
                       (const int*)block_off, (const int*)img_off, (const int*)window, intr, H, W, ray_bid, ray_flat,
                       ray_pix, ray_dir, bid64, flat64, pix64);
    return hipGetLastError();
}
