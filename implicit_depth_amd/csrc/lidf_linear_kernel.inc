// lidf_linear_kernel.inc — the kernel template of lidf_linear.hip, shared with lidf_linear_s / _x / _sx.hip (the SPLIT / XCOL
// instantiations live in translation units of their own: 32 instantiations in one file compiled for two minutes).
#include "lidf_mma.h"

// SPLIT: the operand rows come from TWO buffers — k-quads [0, kq_split) from X, the ones behind them from X2 (the
// joint input gradient of the two decoders on materialised rows: d rows = [S_prob | S_off] [W1_prob ; W1_off], one
// K = 512 product and one store of the [n, 385] rows instead of two K = 256 products, two stores and autograd's add)
// XCOL: one more output column behind the NT tiles (385 = 12 x 32 + 1: a thirteenth tile would multiply 31 columns of
// zeros) through the vector unit — its weights ride as one more quad per k-quad of the stream (the same four values
// for every row lane of a half-wave), 4 FMAs per lane and k-quad beside 4 NT matrix instructions; plain store or
// accumulate, no other epilogue.
template <int NT, bool SPLIT, bool XCOL>
__global__ void __launch_bounds__(256) lidf_linear_kernel(LinearArgs a) {
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int h = lane >> 5;
    const int col = lane & 31;
    // a.nt_total > 0: the launch is split over the output tiles (grid.y = tile; NT = 1): a layer over a
    // handful of rows (the per-voxel layers of the PointNet: 74 rows x 256 outputs) is one wavefront's
    // chain of NT x 4 matrix instructions per k-quad otherwise — 8 workgroups side by side instead
    const int NTS = a.nt_total > 0 ? a.nt_total : NT + (XCOL ? 1 : 0);   // quads per k-quad in the stream
    const int T0 = a.nt_total > 0 ? (int)blockIdx.y : 0;   // first output tile of this workgroup
    const __amdgpu_buffer_rsrc_t srs =
        __builtin_amdgcn_make_buffer_rsrc((void*)a.stream, 0, a.kq1 * NTS * 1024, 0x00020000);
    const int vq = lane * 16;
    const long long AN = a.n_dev ? (long long)*a.n_dev : a.n;   // device-side row count (frame path)
    const long long ntile = (AN + 127) / 128;
    // k-quads below kfull hold eight real operand columns for both half-waves: one 16-byte load per lane, no
    // condition. The k-quad(s) behind them carry the row's last columns, the bias and the u column.
    const int kfull = a.D / 8 < a.kq1 ? a.D / 8 : a.kq1;
    // Operand registers live across the tile loop: the next tile's first loads are issued in FRONT of this
    // tile's stores (vector memory completes in order — a load behind 32 stores waits for their acknowledgements,
    // docs/history.md §4.5), so the first matrix instruction of a tile waits for two loads, not for the previous
    // tile's output to reach memory.
    float b0[4], b1[4], b2[4], b3[4];   // operand ring: k-quads kq, kq + 1, (kq + 2, kq + 3)
    f32x4 q0[NT], q1[NT];               // weight quads of k-quad kq, kq + 1
    f32x4 x0 = {0.f, 0.f, 0.f, 0.f}, x1 = {0.f, 0.f, 0.f, 0.f};   // XCOL: the extra column's weights of kq, kq + 1
    const float* xrow = nullptr;
    const float* xrow2 = nullptr;   // SPLIT: the second buffer's row, biased by -8 kq_split
    long long pc = 0;
    auto load_b_fast = [&](int kq, float (&b)[4]) {
        const float* xr = xrow;
        if (SPLIT) xr = kq >= a.kq_split ? xrow2 : xrow;   // (kq wave-uniform)
        const f32x4u v = *(const f32x4u*)(xr + 8 * kq);
        b[0] = v[0]; b[1] = v[1]; b[2] = v[2]; b[3] = v[3];
    };
    auto load_b_tail = [&](int kq, float (&b)[4]) {
        const int x0 = 8 * kq + 4 * h;
#pragma unroll
        for (int jj = 0; jj < 4; ++jj)
            b[jj] = x0 + jj < a.D ? xrow[8 * kq + jj]
                                  : ((x0 + jj == a.D && a.has_bias)
                                         ? 1.f
                                         : ((x0 + jj == a.D + 1 && a.xoff) ? a.xoff[pc] : 0.f));
    };
    auto load_b = [&](int kq, float (&b)[4]) {   // (kq wave-uniform)
        if (kq < kfull) load_b_fast(kq, b);
        else if (kq < a.kq1) load_b_tail(kq, b);
        else { b[0] = 0.f; b[1] = 0.f; b[2] = 0.f; b[3] = 0.f; }
    };
    auto load_q = [&](int kq, f32x4 (&q)[NT], f32x4& qx) {
#pragma unroll
        for (int t = 0; t < NT; ++t) q[t] = LDQ(srs, vq, (kq * NTS + T0 + t) * 1024);
        if (XCOL) qx = LDQ(srs, vq, (kq * NTS + NT) * 1024);
    };
    // rows of a tile for this lane; the tile's first requests: operands of k-quads 0 and 1, weight quads of k-quad 0
    auto tile_begin = [&](long long tile) {
        const long long p = tile * 128 + wave * 32 + col;
        pc = p < AN ? p : AN - 1;
        xrow = a.X + (size_t)pc * a.ldx + 4 * h;
        if (SPLIT) xrow2 = a.X2 + (size_t)pc * a.ldx2 + 4 * h - 8 * (long long)a.kq_split;
        load_b(0, b0);
        load_b(1, b1);
        load_q(0, q0, x0);
    };
    long long tile = blockIdx.x;
    if (tile < ntile && tile * 128 + wave * 32 < AN) tile_begin(tile);
    for (; tile < ntile; tile += gridDim.x) {
        if (tile * 128 + wave * 32 >= AN) continue;   // (only the last tile can be short: no later tile for this wave)
        const long long p = tile * 128 + wave * 32 + col;
        const bool valid = p < AN;
        f32x16 acc[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) {
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[t][i] = 0.f;
        }
        float xacc = 0.f;
        auto mfma_quad = [&](const f32x4 (&q)[NT], const f32x4& qx, const float (&b)[4]) {
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                f32x16 c = acc[t];
                c = MFMA(q[t][0], b[0], c);
                c = MFMA(q[t][1], b[1], c);
                c = MFMA(q[t][2], b[2], c);
                c = MFMA(q[t][3], b[3], c);
                acc[t] = c;
            }
            if (XCOL) {
                xacc = __builtin_fmaf(qx[0], b[0], xacc);
                xacc = __builtin_fmaf(qx[1], b[1], xacc);
                xacc = __builtin_fmaf(qx[2], b[2], xacc);
                xacc = __builtin_fmaf(qx[3], b[3], xacc);
            }
        };
        int kq = 0;
        // main loop, four k-quads per trip through a ring of four operand sets and two weight sets (no copies):
        // the operand of k-quad kq + 2 and the weight quads of kq + 1 are requested BEFORE the 4 NT matrix
        // instructions of k-quad kq — the operand rows come from HBM (two k-quads of matrix time ahead), the
        // weight quads from L2 (one ahead). Left to itself the compiler sinks the requests behind the products
        // and every k-quad starts on a memory round trip.
        for (; kq + 5 < kfull; kq += 4) {
            load_b_fast(kq + 2, b2); load_q(kq + 1, q1, x1); SCHED_FENCE(); mfma_quad(q0, x0, b0); SCHED_FENCE();
            load_b_fast(kq + 3, b3); load_q(kq + 2, q0, x0); SCHED_FENCE(); mfma_quad(q1, x1, b1); SCHED_FENCE();
            load_b_fast(kq + 4, b0); load_q(kq + 3, q1, x1); SCHED_FENCE(); mfma_quad(q0, x0, b2); SCHED_FENCE();
            load_b_fast(kq + 5, b1); load_q(kq + 4, q0, x0); SCHED_FENCE(); mfma_quad(q1, x1, b3); SCHED_FENCE();
        }
        // the last k-quads (at most five whole ones + the tail k-quads), one per trip with register copies
        for (; kq < a.kq1; ++kq) {
            load_b(kq + 2, b2);
            load_q(kq + 1 < a.kq1 ? kq + 1 : kq, q1, x1);
            SCHED_FENCE();
            mfma_quad(q0, x0, b0);
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) { b0[jj] = b1[jj]; b1[jj] = b2[jj]; }
#pragma unroll
            for (int t = 0; t < NT; ++t) q0[t] = q1[t];
            if (XCOL) x0 = x1;
            SCHED_FENCE();
        }
        // the next tile's first requests, in front of this tile's stores
        {
            const long long nx = tile + gridDim.x;
            if (nx < ntile && nx * 128 + wave * 32 < AN) tile_begin(nx);
            SCHED_FENCE();
        }
        // ---- epilogue: this lane holds, per tile t and group g, features 32t + 8g + 4h + {0..3}
        // a negative index = this row takes no part (its gathered term is absent, it is not pooled)
        const int ai = (valid && a.addrows) ? a.addidx[p] : -1;
        const float* ar = ai >= 0 ? a.addrows + (size_t)ai * a.ld_add + 4 * h : nullptr;
        const float* ar2 =
            (valid && a.addrows2) ? a.addrows2 + (size_t)a.addidx2[p] * a.ld_add2 + 4 * h : nullptr;
        float* op = (valid && a.out) ? a.out + (size_t)p * a.ld_out + 4 * h : nullptr;
        if (XCOL) {   // the two half-waves hold the two halves of every k-quad's products
            const float tot = xacc + __shfl_xor(xacc, 32);
            if (valid && h == 0 && a.out) {
                float* q = a.out + (size_t)p * a.ld_out + 32 * NT;
                *q = a.accumulate ? *q + tot : tot;
            }
        }
        const float* mp = (valid && a.mask_src) ? a.mask_src + (size_t)p * a.ld_mask + 4 * h : nullptr;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                f32x4 v;
#pragma unroll
                for (int i = 0; i < 4; ++i) v[i] = acc[t][4 * g + i];
                // (a.nout > 0: columns >= nout are padding of the last tile — no gathered term is read
                // for them, they are neither stored nor pooled)
                const int cg = (T0 + t) * 32 + 8 * g + 4 * h;
                const bool whole = a.nout <= 0 || cg + 3 < a.nout;
                if (ar) {
                    if (whole) {
                        const f32x4 r = *(const f32x4*)(ar + (T0 + t) * 32 + 8 * g);
#pragma unroll
                        for (int i = 0; i < 4; ++i) v[i] += r[i];
                    } else {
#pragma unroll
                        for (int i = 0; i < 4; ++i)
                            if (cg + i < a.nout) v[i] += ar[(T0 + t) * 32 + 8 * g + i];
                    }
                }
                if (ar2) {
                    if (whole) {
                        const f32x4 r = *(const f32x4*)(ar2 + (T0 + t) * 32 + 8 * g);
#pragma unroll
                        for (int i = 0; i < 4; ++i) v[i] += r[i];
                    } else {
#pragma unroll
                        for (int i = 0; i < 4; ++i)
                            if (cg + i < a.nout) v[i] += ar2[(T0 + t) * 32 + 8 * g + i];
                    }
                }
                if (a.relu) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) v[i] = fmaxf(v[i], a.slope * v[i]);
                }
                const int c0 = (T0 + t) * 32 + 8 * g + 4 * h;  // first of this lane's four columns
                if (mp && (a.nout <= 0 || c0 + 3 < a.nout)) {
                    // dgrad through a leaky ReLU: the activation's output has the sign of its input
                    const f32x4 m = *(const f32x4*)(mp + (T0 + t) * 32 + 8 * g);
#pragma unroll
                    for (int i = 0; i < 4; ++i) v[i] *= m[i] > 0.f ? 1.f : a.mask_slope;
                } else if (mp && c0 < a.nout) {
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        if (c0 + i < a.nout) v[i] *= mp[(T0 + t) * 32 + 8 * g + i] > 0.f ? 1.f : a.mask_slope;
                }
                if (op) {
                    if (a.nout <= 0 || c0 + 3 < a.nout) {
                        if (a.accumulate) {
                            const f32x4 o = *(const f32x4*)(op + (T0 + t) * 32 + 8 * g);
#pragma unroll
                            for (int i = 0; i < 4; ++i) v[i] += o[i];
                        }
                        *(f32x4*)(op + (T0 + t) * 32 + 8 * g) = v;
                    } else {
#pragma unroll
                        for (int i = 0; i < 4; ++i)
                            if (c0 + i < a.nout) {
                                float* q = op + (T0 + t) * 32 + 8 * g + i;
                                *q = a.accumulate ? *q + v[i] : v[i];
                            }
                    }
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[t][4 * g + i] = v[i];
            }
        }
        if (a.pool) {
            // max-pool into pool[poolidx[row]] (values are post-ReLU, >= 0, pool starts at 0).
            // Neighbouring rows mostly share their voxel, so the wave first reduces per distinct
            // voxel: members keep their value, the others contribute 0 (the identity), a 5-step
            // shuffle max over the 32 row lanes of each half, and one lane issues the atomics —
            // and only where a plain (possibly stale; entries only grow) read does not already
            // prove them unnecessary. More than 4 distinct voxels: per-lane atomics.
            const int vox = valid ? a.poolidx[p] : -1;
            unsigned todo = (unsigned)__ballot(valid && h == 0 && vox >= 0);
            int rounds = 0;
            while (todo && rounds < 4) {
                const int lead = __builtin_ctz(todo);
                const int vv = __builtin_amdgcn_readlane(vox, lead);
                const unsigned mem = (unsigned)__ballot(vox == vv) & todo;
                todo &= ~mem;
                ++rounds;
                const bool mine = vox == vv;
                int* pp = (int*)a.pool + (size_t)vv * a.ld_pool + 4 * h;
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    if (a.nout > 0 && (T0 + t) * 32 >= a.nout) continue;   // padding tile (wave-uniform)
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        f32x4 m;
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            float x = mine ? acc[t][4 * g + i] : 0.f;
#pragma unroll
                            for (int sft = 16; sft >= 1; sft >>= 1) x = fmaxf(x, __shfl_xor(x, sft));
                            m[i] = x;
                        }
                        if (col == lead) {
                            const f32x4 seen = *(const f32x4*)(pp + (T0 + t) * 32 + 8 * g);
#pragma unroll
                            for (int i = 0; i < 4; ++i)
                                if (m[i] > seen[i])
                                    atomicMax(pp + (T0 + t) * 32 + 8 * g + i, __float_as_int(m[i]));
                        }
                    }
                }
            }
            if (todo && valid && ((todo >> col) & 1u)) {
                int* pp = (int*)a.pool + (size_t)vox * a.ld_pool + 4 * h;
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    if (a.nout > 0 && (T0 + t) * 32 >= a.nout) continue;
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const f32x4 seen = *(const f32x4*)(pp + (T0 + t) * 32 + 8 * g);
#pragma unroll
                        for (int i = 0; i < 4; ++i)
                            if (acc[t][4 * g + i] > seen[i])
                                atomicMax(pp + (T0 + t) * 32 + 8 * g + i, __float_as_int(acc[t][4 * g + i]));
                    }
                }
            }
        }
    }
}

template <bool SPLIT, bool XCOL>
static void launch_linear_nt(int nt, dim3 g, dim3 b, hipStream_t st, const LinearArgs& a) {
    switch (nt) {
        case 1: hipLaunchKernelGGL((lidf_linear_kernel<1, SPLIT, XCOL>), g, b, 0, st, a); break;
        case 2: hipLaunchKernelGGL((lidf_linear_kernel<2, SPLIT, XCOL>), g, b, 0, st, a); break;
        case 3: hipLaunchKernelGGL((lidf_linear_kernel<3, SPLIT, XCOL>), g, b, 0, st, a); break;
        case 4: hipLaunchKernelGGL((lidf_linear_kernel<4, SPLIT, XCOL>), g, b, 0, st, a); break;
        case 5: hipLaunchKernelGGL((lidf_linear_kernel<5, SPLIT, XCOL>), g, b, 0, st, a); break;
        case 6: hipLaunchKernelGGL((lidf_linear_kernel<6, SPLIT, XCOL>), g, b, 0, st, a); break;
        case 7: hipLaunchKernelGGL((lidf_linear_kernel<7, SPLIT, XCOL>), g, b, 0, st, a); break;
        default: hipLaunchKernelGGL((lidf_linear_kernel<8, SPLIT, XCOL>), g, b, 0, st, a); break;
    }
}
