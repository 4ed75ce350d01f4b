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

struct PnetActC {   // the block the forward keeps for the backward (sorted-order rows)
    float* inps;
    int* voxs;
    float *f1s, *f2s, *f4s, *pool1;
    int* arg1;
    float *g1, *pool2;
    int* arg2;
    float* out;
    int *vstart, *first;
    char* sort;
};
static PnetActC pnetc_act(Carver& c, int64_t n, int64_t v) {
    PnetActC a;
    const size_t N = (size_t)(n > 0 ? n : 1), V = (size_t)(v > 0 ? v : 1);
    a.inps = c.take<float>(N * 6);
    a.voxs = c.take<int>(N);
    a.f1s = c.take<float>(N * 32);
    a.f2s = c.take<float>(N * 64);
    a.f4s = c.take<float>(N * 128);
    a.pool1 = c.take<float>(V * 64);
    a.arg1 = c.take<int>(V * 64);
    a.g1 = c.take<float>(V * 64);
    a.pool2 = c.take<float>(V * 128);
    a.arg2 = c.take<int>(V * 128);
    a.out = c.take<float>(V * 128);
    a.vstart = c.take<int>(V + 2);
    a.first = c.take<int>(V + 2);
    a.sort = (char*)c.take_bytes(lidf_sort_idx_ws_bytes((long long)N, (long long)V));
    return a;
}
struct PnetWsC {   // scratch of one forward / backward
    char* pool64;
    float *gpart, *dz_out, *dp2, *dz4s, *df2s, *partial, *s4, *dg1, *dp1, *dz2s, *dz1s, *wg, *stream;
};
static PnetWsC pnetc_ws(Carver& c, int64_t n, int64_t v) {
    PnetWsC w;
    const size_t N = (size_t)(n > 0 ? n : 1), V = (size_t)(v > 0 ? v : 1);
    w.pool64 = c.take<char>(V * (64 + 128) * 8);
    w.gpart = c.take<float>(V * 128);
    w.dz_out = c.take<float>(V * 128);
    w.dp2 = c.take<float>(V * 128);
    w.dz4s = c.take<float>(N * 128);
    w.df2s = c.take<float>(N * 64);
    w.partial = c.take<float>((N / (size_t)lidf_pnet_chunk_rows() + V + 1) * 128);
    w.s4 = c.take<float>(V * 128);
    w.dg1 = c.take<float>(V * 64);
    w.dp1 = c.take<float>(V * 64);
    w.dz2s = c.take<float>(N * 64);
    w.dz1s = c.take<float>(N * 32);
    w.wg = c.take<float>(WG_SCRATCH_FLOATS);
    w.stream = (float*)c.take_bytes(linex_stream_bytes(256));
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
static int pnetc_forward(const float* inp, const int32_t* vox, int64_t n, int64_t V, float* out, const PnetActC& a,
                         const PnetWsC& w, const float* chain, float* const streams[7], int cus, hipStream_t st) {
    int rc;
    {
        float* zp[1] = {(float*)w.pool64};
        const long long zc[1] = {(long long)V * (64 + 128) * 2};
        CHECK_HIP(lidf_launch_zero_segments(zp, zc, 1, st));
    }
    const int *perm = nullptr, *n_perm = nullptr;
    CHECK_HIP(lidf_launch_sort_idx(vox, n, nullptr, V, a.sort, &perm, &n_perm, st));
    size_t sc_off, perm_off;
    int nblk;
    lidf_sort_idx_layout(n, V, &sc_off, &nblk, &perm_off);
    CHECK_HIP(lidf_launch_pnet_tables((const int*)(a.sort + sc_off), nblk, V, n_perm, a.vstart, a.first, st));
    float *gpart = w.gpart, *pool1 = a.pool1, *g1 = a.g1, *pool2 = a.pool2;
    void* p64_1 = w.pool64;
    void* p64_2 = w.pool64 + (size_t)V * 64 * 8;
    CHECK_HIP(lidf_launch_pnet_train_fwd(1, chain, inp, vox, perm, n_perm, nullptr, a.inps, a.voxs, a.f1s, a.f2s,
                                         nullptr, p64_1, V, n, cus, st));
    CHECK_HIP(lidf_launch_pnet_unpack(p64_1, V * 64, pool1, a.arg1, st));
    // g1 = relu(vox_lin1(pool1)); gpart[v] = W3[:, :64] g1[v] + b3: one launch over the voxels
    if ((rc = run_vox2(pool1, 64, V, nullptr, streams[2], 2, 1, g1, streams[3], 9, 4, 0, gpart, st))) return rc;
    CHECK_HIP(lidf_launch_pnet_train_fwd(2, chain, inp, vox, perm, n_perm, gpart, nullptr, nullptr, nullptr, nullptr,
                                         a.f4s, p64_2, V, n, cus, st));
    CHECK_HIP(lidf_launch_pnet_unpack(p64_2, V * 128, pool2, a.arg2, st));
    // out = relu(vox_lin2(pool2))
    float* outk = a.out;
    if ((rc = run_vox2(pool2, 128, V, nullptr, streams[6], 4, 1, outk, nullptr, 0, 0, 0, nullptr, st))) return rc;
    if (out && out != outk)
        CHECK_HIP(hipMemcpyAsync(out, outk, (size_t)V * 128 * 4, hipMemcpyDeviceToDevice, st));
    return LIDF_OK;
}

// backward: slots = the seven transposed-launch streams of pointnet_backward_impl (0: vox_lin2^T, 3: the voxel half
// of point_lin3^T, 4: vox_lin1^T are the ones read here), pack_mode 0 = pack and run, 2 = packed earlier (then
// `slots` must be given); bwd = the backward chains' stream. Parameter gradients are accumulated into.
static int pnetc_backward(const LidfPointNet* w, int64_t n, int64_t V, const PnetActC& a, const float* g_out,
                          float* d_inp, bool zero_dinp, const LidfPointNetGrads* g, const PnetWsC& s,
                          float* const* slots, int pack_mode, const float* bwd, int cus, hipStream_t st) {
    int rc;
    size_t sc_off, perm_off;
    int nblk;
    lidf_sort_idx_layout(n, V, &sc_off, &nblk, &perm_off);   // (where the forward's sort left its scan and perm)
    const int* scanned = (const int*)(a.sort + sc_off);
    const int* n_perm = scanned + (size_t)V * nblk;
    const int* perm = (const int*)(a.sort + perm_off);
    const float *inps = a.inps, *f1s = a.f1s, *f2s = a.f2s, *f4s = a.f4s;
    const int* voxs = a.voxs;
    const float *pool1 = a.pool1, *g1 = a.g1, *pool2 = a.pool2, *outv = a.out;
    const int *arg1 = a.arg1, *arg2 = a.arg2, *vstart = a.vstart, *first = a.first;
    float *dz_out = s.dz_out, *dp2 = s.dp2, *dz4s = s.dz4s, *df2s = s.df2s, *s4 = s.s4, *dg1 = s.dg1, *dp1 = s.dp1,
          *dz2s = s.dz2s, *dz1s = s.dz1s, *wgs = s.wg, *sbuf = s.stream;
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
    CHECK_HIP(lidf_launch_pnet_segsum(dz4s, vstart, first, V, n, s.partial, s4, st));
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
struct PnetPubWs { PnetWsC scratch; float *chain, *bwd, *s[7]; };
static PnetPubWs pnet_pub_ws(Carver& c, int64_t n, int64_t v) {
    PnetPubWs w;
    w.scratch = pnetc_ws(c, n, v);
    w.chain = (float*)c.take_bytes(lidf_pointnet_chain_stream_bytes());
    w.bwd = (float*)c.take_bytes(PNETC_BWD_STREAM_BYTES);
    pnet_streams(c, w.s);
    return w;
}
// (either path's needs: which one a call takes, pnetc_ok decides)
LIDF_API size_t lidf_pointnet_train_act_floats(int64_t n_pts, int64_t n_vox) {
    Carver c(nullptr, 4);
    c.either([&](Carver& u) { pnet_act(u, n_pts, n_vox); },
             [&](Carver& u) { Carver k; pnetc_act(k, n_pts, n_vox); u.take_bytes(k.used()); });
    return c.used() / sizeof(float);
}
LIDF_API size_t lidf_pointnet_train_workspace_bytes(int64_t n_pts, int64_t n_vox) {
    Carver c;
    c.either([&](Carver& u) { pnet_train_ws(u, n_pts, n_vox); }, [&](Carver& u) { pnet_pub_ws(u, n_pts, n_vox); });
    return c.used();
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
    Carver c(workspace), ca(act);
    const PnetPubWs pw = pnet_pub_ws(c, n, n_vox);
    CHECK_CARVED(c, workspace, workspace_bytes);
    if ((rc = cu_count(&cus))) return rc;
    hipStream_t st = (hipStream_t)stream;
    if ((rc = pnetc_pack(w, pw.chain, pw.s, pw.bwd, cus, st))) return rc;
    return pnetc_forward(inp, vox, n, n_vox, out, pnetc_act(ca, n, n_vox), pw.scratch, pw.chain, pw.s, cus, st);
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
    Carver c(workspace), ca(act);
    const PnetPubWs pw = pnet_pub_ws(c, n, n_vox);
    CHECK_CARVED(c, workspace, workspace_bytes);
    if ((rc = cu_count(&cus))) return rc;
    hipStream_t st = (hipStream_t)stream;
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
        CHECK_HIP(pack_stream(lay, nw, nw, m0, pw.bwd, nullptr, st));
    }
    (void)inp; (void)vox;   // (the forward kept their sorted copies)
    return pnetc_backward(w, n, n_vox, pnetc_act(ca, n, n_vox), g_out, d_inp, true, g, pw.scratch, nullptr, 0, pw.bwd,
                          cus, st);
}
