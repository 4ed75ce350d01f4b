// lidf_api_pointnet_train.inc — PointNet2Stage under autograd through the register chains of
// lidf_pointnet_train.hip (included by lidf_api.hip behind the layer-by-layer training path, which stays as the
// path for voxel tables beyond the sort's 16,384 rows and as the A/B reference: LIDF_PNET_TRAIN_CHAIN=0).

static bool pnetc_enabled() {
    static int on = -1;
    if (on < 0) {
        const char* e = getenv("LIDF_PNET_TRAIN_CHAIN");
        on = (e && e[0] == '0') ? 0 : 1;
    }
    return on == 1;
}
// the chains walk the points grouped by voxel: the stable counting sort holds a block's histogram in LDS
static bool pnetc_ok(int64_t n, int64_t V) {
    return pnetc_enabled() && n > 0 && V > 0 && V <= 16384 && n <= 0x7fffffffLL / 128 &&
           lidf_sort_idx_ws_bytes(n, V) > 0;
}

struct PnetActC {   // byte offsets into the block the forward keeps for the backward (sorted-order rows)
    size_t inps, voxs, f1s, f2s, f4s, pool1, arg1, g1, pool2, arg2, out, vstart, first, sort, total;
};
static PnetActC pnetc_act(int64_t n, int64_t v) {
    PnetActC a;
    const size_t N = (size_t)(n > 0 ? n : 1), V = (size_t)(v > 0 ? v : 1);
    size_t o = 0;
    a.inps = o;   o += align_up(N * 24, 256);
    a.voxs = o;   o += align_up(N * 4, 256);
    a.f1s = o;    o += align_up(N * 32 * 4, 256);
    a.f2s = o;    o += align_up(N * 64 * 4, 256);
    a.f4s = o;    o += align_up(N * 128 * 4, 256);
    a.pool1 = o;  o += align_up(V * 64 * 4, 256);
    a.arg1 = o;   o += align_up(V * 64 * 4, 256);
    a.g1 = o;     o += align_up(V * 64 * 4, 256);
    a.pool2 = o;  o += align_up(V * 128 * 4, 256);
    a.arg2 = o;   o += align_up(V * 128 * 4, 256);
    a.out = o;    o += align_up(V * 128 * 4, 256);
    a.vstart = o; o += align_up((V + 2) * 4, 256);
    a.first = o;  o += align_up((V + 2) * 4, 256);
    a.sort = o;   o += align_up(lidf_sort_idx_ws_bytes((long long)N, (long long)V), 256);
    a.total = o;
    return a;
}
struct PnetWsC {   // scratch of one forward / backward
    size_t pool64, gpart, dz_out, dp2, dz4s, df2s, partial, s4, dg1, dp1, dz2s, dz1s, wg, stream, total;
};
static PnetWsC pnetc_ws(int64_t n, int64_t v) {
    PnetWsC w;
    const size_t N = (size_t)(n > 0 ? n : 1), V = (size_t)(v > 0 ? v : 1);
    size_t o = 0;
    w.pool64 = o;  o += align_up(V * (64 + 128) * 8, 256);
    w.gpart = o;   o += align_up(V * 128 * 4, 256);
    w.dz_out = o;  o += align_up(V * 128 * 4, 256);
    w.dp2 = o;     o += align_up(V * 128 * 4, 256);
    w.dz4s = o;    o += align_up(N * 128 * 4, 256);
    w.df2s = o;    o += align_up(N * 64 * 4, 256);
    w.partial = o; o += align_up((N / (size_t)lidf_pnet_chunk_rows() + V + 1) * 128 * 4, 256);
    w.s4 = o;      o += align_up(V * 128 * 4, 256);
    w.dg1 = o;     o += align_up(V * 64 * 4, 256);
    w.dp1 = o;     o += align_up(V * 64 * 4, 256);
    w.dz2s = o;    o += align_up(N * 64 * 4, 256);
    w.dz1s = o;    o += align_up(N * 32 * 4, 256);
    w.wg = o;      o += align_up(WG_SCRATCH_FLOATS * 4, 256);
    w.stream = o;  o += linex_stream_bytes(256);
    w.total = o;
    return w;
}
#define PNETC_BWD_STREAM_BYTES ((size_t)(PNB_A_QUADS + PNB_B_QUADS) * 1024)

// the streams the chains read: the inference chains' stream + the per-voxel layers' (vox_lin1, the voxel half of
// point_lin3 with its bias, vox_lin2: slots 2, 3, 6 as pointnet_impl's inference branch packs them) + the backward
// chains' stream. Pack jobs of the caller's JobScope, or direct launches without one.
static int pnetc_pack(const LidfPointNet* w, float* chain, float* const streams[7], float* bwd, int cus,
                      hipStream_t st) {
    PnetBufs b = {};
    for (int i = 0; i < 7; ++i) b.streams[i] = streams[i];
    b.chain = chain;
    int rc;
    if ((rc = pointnet_impl(w, nullptr, nullptr, 0, 0, nullptr, b, cus, st, 1))) return rc;
    StreamLayout lay = {};
    lay.nets = 1; lay.mode = LIDF_MODE_PNET_BWD;
    lay.total = (int)(PNETC_BWD_STREAM_BYTES / 4);
    NetW nw = {};
    nw.w1 = w->w_p1; nw.b1 = w->b_p1; nw.w2 = w->w_p2; nw.b2 = w->b_p2; nw.w3 = w->w_p3;
    nw.b3 = w->w_p4; nw.w4 = w->b_p4;
    L1Map m0 = {};
    CHECK_HIP(pack_stream(lay, nw, nw, m0, bwd, nullptr, st));
    return LIDF_OK;
}

// forward with what the backward needs kept in `act` (pnetc_act); streams packed by pnetc_pack
static int pnetc_forward(const float* inp, const int32_t* vox, int64_t n, int64_t V, float* out, char* act,
                         char* ws, const float* chain, float* const streams[7], int cus, hipStream_t st) {
    int rc;
    const PnetActC a = pnetc_act(n, V);
    const PnetWsC w = pnetc_ws(n, V);
    float* pool64 = (float*)(ws + w.pool64);
    {
        float* zp[1] = {pool64};
        const long long zc[1] = {(long long)V * (64 + 128) * 2};
        CHECK_HIP(lidf_launch_zero_segments(zp, zc, 1, st));
    }
    const int *perm = nullptr, *n_perm = nullptr;
    CHECK_HIP(lidf_launch_sort_idx(vox, n, nullptr, V, act + a.sort, &perm, &n_perm, st));
    size_t sc_off, perm_off;
    int nblk;
    lidf_sort_idx_layout(n, V, &sc_off, &nblk, &perm_off);
    int* vstart = (int*)(act + a.vstart);
    int* first = (int*)(act + a.first);
    CHECK_HIP(lidf_launch_pnet_tables((const int*)(act + a.sort + sc_off), nblk, V, n_perm, vstart, first, st));
    float* gpart = (float*)(ws + w.gpart);
    float *pool1 = (float*)(act + a.pool1), *g1 = (float*)(act + a.g1), *pool2 = (float*)(act + a.pool2);
    void* p64_1 = ws + w.pool64;
    void* p64_2 = ws + w.pool64 + (size_t)V * 64 * 8;
    CHECK_HIP(lidf_launch_pnet_train_fwd(1, chain, inp, vox, perm, n_perm, nullptr, (float*)(act + a.inps),
                                         (int*)(act + a.voxs), (float*)(act + a.f1s), (float*)(act + a.f2s), nullptr,
                                         p64_1, V, n, cus, st));
    CHECK_HIP(lidf_launch_pnet_unpack(p64_1, V * 64, pool1, (int*)(act + a.arg1), st));
    // g1 = relu(vox_lin1(pool1)); gpart[v] = W3[:, :64] g1[v] + b3: one launch over the voxels
    if ((rc = run_vox2(pool1, 64, V, nullptr, streams[2], 2, 1, g1, streams[3], 9, 4, 0, gpart, st))) return rc;
    CHECK_HIP(lidf_launch_pnet_train_fwd(2, chain, inp, vox, perm, n_perm, gpart, nullptr, nullptr, nullptr, nullptr,
                                         (float*)(act + a.f4s), p64_2, V, n, cus, st));
    CHECK_HIP(lidf_launch_pnet_unpack(p64_2, V * 128, pool2, (int*)(act + a.arg2), st));
    // out = relu(vox_lin2(pool2))
    float* outk = (float*)(act + a.out);
    if ((rc = run_vox2(pool2, 128, V, nullptr, streams[6], 4, 1, outk, nullptr, 0, 0, 0, nullptr, st))) return rc;
    if (out && out != outk)
        CHECK_HIP(hipMemcpyAsync(out, outk, (size_t)V * 128 * 4, hipMemcpyDeviceToDevice, st));
    return LIDF_OK;
}

// backward: slots = the seven transposed-launch streams of pointnet_backward_impl (0: vox_lin2^T, 3: the voxel half
// of point_lin3^T, 4: vox_lin1^T are the ones read here), pack_mode 0 = pack and run, 2 = packed earlier (then
// `slots` must be given); bwd = the backward chains' stream. Parameter gradients are accumulated into.
static int pnetc_backward(const LidfPointNet* w, int64_t n, int64_t V, const char* act, const float* g_out,
                          float* d_inp, bool zero_dinp, const LidfPointNetGrads* g, char* ws, float* const* slots,
                          int pack_mode, const float* bwd, int cus, hipStream_t st) {
    int rc;
    const PnetActC a = pnetc_act(n, V);
    const PnetWsC s = pnetc_ws(n, V);
    size_t sc_off, perm_off;
    int nblk;
    lidf_sort_idx_layout(n, V, &sc_off, &nblk, &perm_off);   // (where the forward's sort left its scan and perm)
    const int* scanned = (const int*)(act + a.sort + sc_off);
    const int* n_perm = scanned + (size_t)V * nblk;
    const int* perm = (const int*)(act + a.sort + perm_off);
    const float *inps = (const float*)(act + a.inps), *f1s = (const float*)(act + a.f1s);
    const float *f2s = (const float*)(act + a.f2s), *f4s = (const float*)(act + a.f4s);
    const int* voxs = (const int*)(act + a.voxs);
    const float *pool1 = (const float*)(act + a.pool1), *g1 = (const float*)(act + a.g1);
    const float *pool2 = (const float*)(act + a.pool2), *outv = (const float*)(act + a.out);
    const int *arg1 = (const int*)(act + a.arg1), *arg2 = (const int*)(act + a.arg2);
    const int *vstart = (const int*)(act + a.vstart), *first = (const int*)(act + a.first);
    float* dz_out = (float*)(ws + s.dz_out);
    float* dp2 = (float*)(ws + s.dp2);
    float* dz4s = (float*)(ws + s.dz4s);
    float* df2s = (float*)(ws + s.df2s);
    float* s4 = (float*)(ws + s.s4);
    float* dg1 = (float*)(ws + s.dg1);
    float* dp1 = (float*)(ws + s.dp1);
    float* dz2s = (float*)(ws + s.dz2s);
    float* dz1s = (float*)(ws + s.dz1s);
    float* wgs = (float*)(ws + s.wg);
    float* sbuf = (float*)(ws + s.stream);
    auto lin = [&](const LinEx& L, int slot) {
        return run_linex(L, slots ? slots[slot] : sbuf, cus, st, slots ? pack_mode : 0);
    };
    if (d_inp && zero_dinp) CHECK_HIP(hipMemsetAsync(d_inp, 0, (size_t)n * 24, st));
    // out = relu(vox_lin2(pool2))
    CHECK_HIP(lidf_launch_relu_mask(g_out, outv, V * 128, dz_out, st));
    CHECK_HIP(lidf_launch_wgrad(dz_out, 128, 128, pool2, 128, 128, V, g->w_v2, 128, g->b_v2, wgs, WG_SCRATCH_FLOATS, st));
    LinEx L = {};
    L.transposed = 1; L.mask_slope = 0.f;
    L.n = V; L.w = w->w_v2; L.ldw = 128; L.nout = 128; L.k = 128; L.X = dz_out; L.ldx = 128;
    L.out = dp2; L.ld_out = 128;
    if ((rc = lin(L, 0))) return rc;
    // pool2 = segmax(f5), f5 = relu(point_lin4(f4)): dz5 is dp2 at the arg rows and zero elsewhere
    CHECK_HIP(lidf_launch_pnet_dw4(dp2, arg2, f4s, V, g->w_p4, g->b_p4, st));
    CHECK_HIP(lidf_launch_pnet_bwd_a(bwd, voxs, n_perm, dp2, arg2, f4s, dz4s, df2s, n, cus, st));
    // f4 = relu(point_lin3(cat(g1[vox], f2))): weight columns 0..63 meet g1[vox] (per-voxel row sums of dz4),
    // 64..127 meet f2
    CHECK_HIP(lidf_launch_pnet_segsum(dz4s, vstart, first, V, n, (float*)(ws + s.partial), s4, st));
    CHECK_HIP(lidf_launch_wgrad(s4, 128, 128, g1, 64, 64, V, g->w_p3, 128, nullptr, wgs, WG_SCRATCH_FLOATS, st));
    CHECK_HIP(lidf_launch_wgrad(dz4s, 128, 128, f2s, 64, 64, n, g->w_p3 + 64, 128, g->b_p3, wgs, WG_SCRATCH_FLOATS, st));
    // g1 = relu(vox_lin1(pool1))
    L.n = V; L.w = w->w_p3; L.ldw = 128; L.nout = 64; L.k = 128; L.X = s4; L.ldx = 128;
    L.mask_src = g1; L.ld_mask = 64; L.out = dg1; L.ld_out = 64;
    if ((rc = lin(L, 3))) return rc;
    CHECK_HIP(lidf_launch_wgrad(dg1, 64, 64, pool1, 64, 64, V, g->w_v1, 64, g->b_v1, wgs, WG_SCRATCH_FLOATS, st));
    L.mask_src = nullptr;
    L.w = w->w_v1; L.ldw = 64; L.nout = 64; L.k = 64; L.X = dg1; L.ldx = 64; L.out = dp1; L.ld_out = 64;
    if ((rc = lin(L, 4))) return rc;
    // pool1 = segmax(f2): added to the gradient f2 receives through the concat; f2 = relu(point_lin2(f1));
    // f1 = relu(point_lin1(inp))
    CHECK_HIP(lidf_launch_pnet_bwd_b(bwd + (size_t)PNB_A_QUADS * 256, voxs, perm, n_perm, df2s, dp1, arg1, f2s, f1s,
                                     dz2s, dz1s, d_inp, n, cus, st));
    CHECK_HIP(lidf_launch_wgrad(dz2s, 64, 64, f1s, 32, 32, n, g->w_p2, 32, g->b_p2, wgs, WG_SCRATCH_FLOATS, st));
    CHECK_HIP(lidf_launch_wgrad(dz1s, 32, 32, inps, 6, 6, n, g->w_p1, 6, g->b_p1, wgs, WG_SCRATCH_FLOATS, st));
    return LIDF_OK;
}

// ---- the public entry points (include/lidf_hip.h): the chains where the voxel table allows the sort, else layer by
// layer. Workspace of the chains' form: [scratch | inference chains' stream | backward chains' stream | the seven
// layer slots]; every call packs what it reads (the stepwise API keeps no stream between calls).
struct PnetPubWs {
    size_t scratch, chain, bwd, s[7], total;
};
static PnetPubWs pnet_pub_ws(int64_t n, int64_t v) {
    PnetPubWs w;
    size_t o = 0;
    w.scratch = o; o += align_up(pnetc_ws(n, v).total, 256);
    w.chain = o;   o += align_up(lidf_pointnet_chain_stream_bytes(), 256);
    w.bwd = o;     o += align_up(PNETC_BWD_STREAM_BYTES, 256);
    const int ks[7] = {6, 32, 64, 64, 64, 128, 128};
    const int nts[7] = {1, 2, 2, 4, 4, 4, 4};
    for (int i = 0; i < 7; ++i) { w.s[i] = o; o += lin_stream_bytes(ks[i], nts[i]); }
    w.total = o;
    return w;
}
LIDF_API size_t lidf_pointnet_train_act_floats(int64_t n_pts, int64_t n_vox) {
    const size_t a = pnet_act(n_pts, n_vox).total, c = (pnetc_act(n_pts, n_vox).total + 3) / 4;
    return a > c ? a : c;
}
LIDF_API size_t lidf_pointnet_train_workspace_bytes(int64_t n_pts, int64_t n_vox) {
    const size_t a = pnet_train_ws(n_pts, n_vox).total, c = pnet_pub_ws(n_pts, n_vox).total;
    return a > c ? a : c;
}

LIDF_API int lidf_pointnet_forward_train_f32(const LidfPointNet* w, const float* inp, const int32_t* vox, int64_t n,
                                               int64_t n_vox, float* out, float* act, void* workspace,
                                               size_t workspace_bytes, lidf_stream_t stream) {
    if (!w || n < 0 || n_vox < 0) return LIDF_ERR_BAD_ARG;
    if (!pnetc_ok(n, n_vox))
        return pointnet_forward_train_layers(w, inp, vox, n, n_vox, out, act, workspace, workspace_bytes, stream);
    if (!out || !act || !inp || !vox) return LIDF_ERR_BAD_ARG;
    int rc, cus;
    if ((rc = check_pointnet_w(w))) return rc;
    const PnetPubWs pw = pnet_pub_ws(n, n_vox);
    if (!workspace || workspace_bytes < pw.total) return LIDF_ERR_WORKSPACE;
    if ((rc = cu_count(&cus))) return rc;
    char* ws = (char*)workspace;
    float* streams[7];
    for (int i = 0; i < 7; ++i) streams[i] = (float*)(ws + pw.s[i]);
    hipStream_t st = (hipStream_t)stream;
    if ((rc = pnetc_pack(w, (float*)(ws + pw.chain), streams, (float*)(ws + pw.bwd), cus, st))) return rc;
    return pnetc_forward(inp, vox, n, n_vox, out, (char*)act, ws + pw.scratch, (const float*)(ws + pw.chain), streams,
                         cus, st);
}

LIDF_API int lidf_pointnet_backward_f32(const LidfPointNet* w, const float* inp, const int32_t* vox, int64_t n,
                                          int64_t n_vox, const float* act, const float* g_out, float* d_inp,
                                          const LidfPointNetGrads* g, void* workspace, size_t workspace_bytes,
                                          lidf_stream_t stream) {
    if (!w || !g || n < 0 || n_vox < 0) return LIDF_ERR_BAD_ARG;
    if (!pnetc_ok(n, n_vox))
        return pointnet_backward_layers(w, inp, vox, n, n_vox, act, g_out, d_inp, g, workspace, workspace_bytes,
                                        stream);
    int rc, cus;
    if ((rc = check_pointnet_w(w))) return rc;
    if (!g->w_p1 || !g->b_p1 || !g->w_p2 || !g->b_p2 || !g->w_v1 || !g->b_v1 || !g->w_p3 || !g->b_p3 ||
        !g->w_p4 || !g->b_p4 || !g->w_v2 || !g->b_v2 || !act || !g_out)
        return LIDF_ERR_BAD_ARG;
    const PnetPubWs pw = pnet_pub_ws(n, n_vox);
    if (!workspace || workspace_bytes < pw.total) return LIDF_ERR_WORKSPACE;
    if ((rc = cu_count(&cus))) return rc;
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    {   // the gradients start at zero
        float* const zp[12] = {g->w_p1, g->b_p1, g->w_p2, g->b_p2, g->w_v1, g->b_v1, g->w_p3, g->b_p3,
                               g->w_p4, g->b_p4, g->w_v2, g->b_v2};
        const long long zc[12] = {32 * 6, 32, 64 * 32, 64, 64 * 64, 64, 128 * 128, 128, 128 * 128, 128, 128 * 128, 128};
        CHECK_HIP(lidf_launch_zero_segments(zp, zc, 12, st));
    }
    {   // the backward chains' stream (the stepwise API keeps no stream between its calls)
        StreamLayout lay = {};
        lay.nets = 1; lay.mode = LIDF_MODE_PNET_BWD;
        lay.total = (int)(PNETC_BWD_STREAM_BYTES / 4);
        NetW nw = {};
        nw.w1 = w->w_p1; nw.b1 = w->b_p1; nw.w2 = w->w_p2; nw.b2 = w->b_p2; nw.w3 = w->w_p3;
        nw.b3 = w->w_p4; nw.w4 = w->b_p4;
        L1Map m0 = {};
        CHECK_HIP(pack_stream(lay, nw, nw, m0, (float*)(ws + pw.bwd), nullptr, st));
    }
    (void)inp; (void)vox;   // (the forward kept their sorted copies)
    return pnetc_backward(w, n, n_vox, (const char*)act, g_out, d_inp, true, g, ws + pw.scratch, nullptr, 0,
                          (const float*)(ws + pw.bwd), cus, st);
}
