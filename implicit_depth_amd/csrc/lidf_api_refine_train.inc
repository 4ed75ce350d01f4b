// lidf_api_refine_train.inc — stage 2, one training step in two library calls (included at the end of
// lidf_api.hip: it is built from that file's static helpers).
//
// RefineNet.forward 'train' (models/pipeline.py:1032-1041, forward_times x get_pred_refine :922-1030) and the
// backward autograd derives for it (trainers/train_refine.py:393-399). Rounds 3-4 composed this step in Python
// from the modules' own autograd functions, with torch cat / gather / index_add between ~300 launches and the
// decoder on materialised [R,334] rows; here the step is
//   forward : ONE multi-pack of every weight stream (forward and backward launches) | raypart = W1[:, ROI | dir]
//             rayfeat[r] once | per iteration: end voxel + PointNet rows, PointNet2Stage training forward,
//             voxpart = W1[:, 0:128] vox_feat + b1 (+ c), embed(pos) rows, the register-chained decoder that keeps
//             its activations (layer 1 = embed(pos) columns + voxpart[end voxel] + raypart[ray]), position update
//   backward: per iteration in reverse: d off = rs <g, dir>; the factorised decoder backward (chained dgrad,
//             running sum S of dZ1 over the passes, S^T embed(pos), per-voxel segment sums of S -> dW1[:, 0:128],
//             d vox_feat; d embed(pos) = S W1[:, pos columns] only where a gradient has to reach the position);
//             PointNet2Stage backward; adjoint of embed(pos) and of the predicted points' PointNet rows;
//             after the loop the per-ray part once on the sum of S over the iterations.
// Parameter gradients accumulate inside the call (every kernel that writes one adds into it).

// One iteration's block of `act`. The PointNet's forward keeps the chains' sorted rows or the layer-by-layer
// path's activations in the same bytes (pnetc_ok decides which).
struct RtIter {
    float* cur;
    int* end_voxel;
    float* pn_inp;
    int* pn_vox;
    PnetAct pa;
    PnetActC pc;
    float* pe;          // rows [ROI | embed(pos) | embed(dir)]
    float *voxpart, *passes, *pre, *off;
};
static RtIter rt_iter(Carver& c, int64_t R, int64_t Nv, int64_t V, int E, int npass) {
    RtIter l;
    const size_t r = (size_t)(R > 0 ? R : 1), n = (size_t)(R + Nv > 0 ? R + Nv : 1), v = (size_t)(V > 0 ? V : 1);
    l.cur = c.take<float>(r * 3);
    l.end_voxel = c.take<int>(r);
    l.pn_inp = c.take<float>(n * 6);
    l.pn_vox = c.take<int>(n);
    c.either([&](Carver& u) { Carver k = u.here(4); l.pa = pnet_act(k, (int64_t)n, (int64_t)v); u.take_bytes(k.used()); },
             [&](Carver& u) { l.pc = pnetc_act(u, (int64_t)n, (int64_t)v); });
    l.pe = c.take<float>(r * (size_t)(128 + E + 3 + 6 * 16));
    l.voxpart = c.take<float>(v * LIDF_H1);
    l.passes = c.take<float>((size_t)npass * qact_pass((int64_t)r));
    l.pre = c.take<float>(r);
    l.off = c.take<float>(r);
    return l;
}
// `act`: [weight streams | raypart | ray index | per-iteration blocks]
struct RtLay {
    float *s_pnf[7], *s_pnb[PNET_BWD_SLOTS], *s_pnchain, *s_pnbwd, *s_vox, *s_ray;
    char* s_chain;
    float *s_dvox, *s_dpe, *s_dgrad, *raypart;
    int* ray_idx;
    char* iter0;          // T blocks of iter_bytes each (rt_iter)
    size_t iter_bytes;
};
static RtLay rt_lay(Carver& c, int64_t R, int64_t Nv, int64_t V, int E, int npass, int T) {
    RtLay l;
    pnet_streams(c, l.s_pnf);
    for (int i = 0; i < PNET_BWD_SLOTS; ++i) l.s_pnb[i] = (float*)c.take_bytes(linex_stream_bytes(PNET_BWD_SLOT_K[i]));
    l.s_pnchain = (float*)c.take_bytes(lidf_pointnet_chain_stream_bytes());   // the PointNet's chains (forward | backward)
    l.s_pnbwd = (float*)c.take_bytes(PNETC_BWD_STREAM_BYTES);
    l.s_vox = (float*)c.take_bytes(linex_stream_bytes(128));
    l.s_ray = (float*)c.take_bytes(linex_stream_bytes(REFINE_RAY_K));
    l.s_chain = (char*)c.take_bytes(chain_stream_bytes(3 + 6 * 16));
    l.s_dvox = (float*)c.take_bytes(linex_stream_bytes(256));
    l.s_dpe = (float*)c.take_bytes(linex_stream_bytes(256));
    l.s_dgrad = (float*)c.take_bytes(lidf_dgrad_stream_bytes());
    const size_t r = (size_t)(R > 0 ? R : 1);
    l.raypart = c.take<float>(r * LIDF_H1);
    l.ray_idx = c.take<int>(r);
    Carver one;
    rt_iter(one, R, Nv, V, E, npass);
    l.iter_bytes = one.used();
    l.iter0 = (char*)c.take_bytes((size_t)(T > 0 ? T : 1) * l.iter_bytes);
    return l;
}

// the backward's (and the PointNet forward's) scratch
struct RtWs {
    PnetTrainWs pw;     // the PointNet's: layer by layer ...
    PnetWsC pcw;        // ... or through the chains, in the same bytes
    QTrainWs qw;
    float *ssum, *s_it, *dvoxfeat, *d_pe, *d_inp, *g[2], *ss_partial;
};
static RtWs rt_ws(Carver& c, int64_t R, int64_t Nv, int64_t V, int E) {
    RtWs w;
    const size_t r = (size_t)(R > 0 ? R : 1), n = (size_t)(R + Nv > 0 ? R + Nv : 1), v = (size_t)(V > 0 ? V : 1);
    c.either([&](Carver& u) { w.pw = pnet_train_ws(u, (int64_t)n, (int64_t)v); },
             [&](Carver& u) { w.pcw = pnetc_ws(u, (int64_t)n, (int64_t)v); });
    w.qw = qtrain_ws(c, (int64_t)r, (int64_t)r, (int64_t)v);
    w.ssum = c.take<float>(r * LIDF_H1);
    w.s_it = c.take<float>(r * LIDF_H1);
    w.dvoxfeat = c.take<float>(v * 128);
    w.d_pe = c.take<float>(r * (size_t)E);
    w.d_inp = c.take<float>(n * 6);
    w.g[0] = c.take<float>(r * 3);
    w.g[1] = c.take<float>(r * 3);
    c.take<float>(r);   // (a slot no launch uses any more: kept, the workspace's size is part of the ABI's behaviour)
    w.ss_partial = c.take<float>((n / (size_t)lidf_pnet_chunk_rows() + v + 1) * 256);
    return w;
}

LIDF_API size_t lidf_refine_train_act_bytes(int64_t n_rays, int64_t n_valid, int64_t n_vox, int32_t multires,
                                            int32_t multires_views, int32_t n_pass, int32_t forward_times) {
    (void)multires_views;
    if (n_rays < 0 || n_valid < 0 || n_vox < 0 || multires < 0 || multires > 16 || n_pass < 1 || forward_times < 1)
        return 0;
    return carved([&](Carver& c) { rt_lay(c, n_rays, n_valid, n_vox, 3 + 6 * multires, n_pass, forward_times); });
}
LIDF_API size_t lidf_refine_train_workspace_bytes(int64_t n_rays, int64_t n_valid, int64_t n_vox, int32_t multires) {
    if (n_rays < 0 || n_valid < 0 || n_vox < 0 || multires < 0 || multires > 16) return 0;
    return carved([&](Carver& c) { rt_ws(c, n_rays, n_valid, n_vox, 3 + 6 * multires); });
}

static int rt_check(const LidfRefineArgs* q, int T, bool need_out = true) {
    if (!q || T < 1) return LIDF_ERR_BAD_ARG;
    if (q->n_rays < 0 || q->n_valid < 0 || q->n_vox < 0 || q->n_pairs < 0) return LIDF_ERR_BAD_ARG;
    if (q->multires < 0 || q->multires > 16 || q->multires_views < 0 || q->multires_views > 16)
        return LIDF_ERR_UNSUPPORTED;
    if (q->precision != LIDF_PRECISION_F32 || q->pnet_select) return LIDF_ERR_UNSUPPORTED;
    if (q->n_rays > 0x15555555LL || q->n_rays + q->n_valid > 0x15555555LL) return LIDF_ERR_UNSUPPORTED;
    if (!q->off || !q->pnet) return LIDF_ERR_BAD_ARG;
    int rc;
    if ((rc = check_decoder(q->off)) || (rc = check_pointnet_w(q->pnet))) return rc;
    if (q->n_rays == 0) return LIDF_OK;
    if (q->n_vox == 0) return LIDF_ERR_BAD_ARG;
    if (!q->ray_dir || !q->ray_bid || !q->ray_flat || !q->pred_pos || !q->max_pair_id || !q->voxel_bound ||
        !q->voxel_bid || !q->rgb_img || !q->rayfeat || (need_out && !q->pred_pos_out) || (q->n_pairs > 0 && !q->pair_vox) ||
        (q->n_valid > 0 && (!q->valid_inp || !q->valid_vox)))
        return LIDF_ERR_BAD_ARG;
    return LIDF_OK;
}

static int rt_cells(const LidfRefineArgs* q, CellLookup* cells) {
    *cells = {};
    if (!q->voxel_coord) return LIDF_OK;
    if (!q->cell_table || q->batch <= 0 || !(q->grid_part > 0.f)) return LIDF_ERR_BAD_ARG;
    long long nc = q->batch;
    for (int k = 0; k < 3; ++k) {
        if (q->grid_res[k] <= 0) return LIDF_ERR_BAD_ARG;
        cells->g.xmin[k] = q->grid_xmin[k];
        cells->g.r[k] = q->grid_res[k];
        nc *= q->grid_res[k];
    }
    if (nc > 0x7fffffffLL) return LIDF_ERR_UNSUPPORTED;
    cells->g.crop = q->grid_part;
    cells->g.B = q->batch;
    cells->coord = q->voxel_coord;
    cells->table = q->cell_table;
    cells->ready = q->cell_table_ready;
    return LIDF_OK;
}

// the two transposed layer-1 launches of the decoder backward, as qdec_backward_impl builds them (pack only)
static int rt_pack_transposed(const LidfDecoder* dec, int E, int Ed, float* s_dvox, float* s_dpe, int cus,
                              hipStream_t st) {
    int rc;
    const int D = 256 + E + Ed, ld1 = D + (dec->is_ief ? 16 : 0);
    LinEx L = {};
    L.transposed = 1; L.ldw = ld1; L.k = LIDF_H1; L.ldx = LIDF_H1;
    L.w = dec->w1; L.nout = 128; L.ld_out = 128;
    if ((rc = run_linex(L, s_dvox, cus, st, 1))) return rc;
    L.w = dec->w1 + 256; L.nout = E; L.ld_out = E;
    return run_linex(L, s_dpe, cus, st, 1);
}

static void rt_query_args(const LidfRefineArgs* q, const RtLay& l, const RtIter& it, LidfQueryTrainArgs* t) {
    *t = {};
    t->n_pairs = q->n_rays; t->n_rays = q->n_rays; t->n_vox = q->n_vox;
    t->pair_off = nullptr;
    t->pair_ray = l.ray_idx;
    t->pair_vox = it.end_voxel;
    t->pe = it.pe + 128;   // (the embed(pos) window of the iteration's layer-1 rows)
    t->multires = q->multires; t->multires_views = q->multires_views;
    // (occ_voxel_feat of the iteration: where the PointNet's forward keeps its output)
    t->vox_feat = pnetc_ok(q->n_rays + q->n_valid, q->n_vox) ? it.pc.out : it.pa.out;
    t->rayfeat = q->rayfeat;
    t->dec = q->off;
}

LIDF_API int lidf_refine_train_forward_f32(const LidfRefineArgs* q, int32_t forward_times, void* act_v,
                                             size_t act_bytes, lidf_stream_t stream) {
    int rc, cus;
    const int T = forward_times;
    if ((rc = rt_check(q, T))) return rc;
    const int64_t R = q->n_rays, Nv = q->n_valid, V = q->n_vox, P = q->n_pairs, n = R + Nv;
    if (R == 0) return LIDF_OK;
    const LidfDecoder* dec = q->off;
    const int E = 3 + 6 * q->multires, Ed = 3 + 6 * q->multires_views;
    const int npass = dec->is_ief ? dec->n_iter : 1;
    Carver ca(act_v), cw(q->workspace);
    const RtLay l = rt_lay(ca, R, Nv, V, E, npass, T);
    const RtWs w = rt_ws(cw, R, Nv, V, E);
    CHECK_CARVED(ca, act_v, act_bytes);
    CHECK_CARVED(cw, q->workspace, q->workspace_bytes);
    auto iter = [&](int it) {   // block `it` of the per-iteration blocks
        Carver ci(l.iter0 + (size_t)it * l.iter_bytes);
        return rt_iter(ci, R, Nv, V, E, npass);
    };
    CellLookup cells;
    if ((rc = rt_cells(q, &cells))) return rc;
    if ((rc = cu_count(&cus))) return rc;
    hipStream_t st = (hipStream_t)stream;
    const bool chain = pnetc_ok(n, V);   // PointNet2Stage through the training chains (else layer by layer)
    float* const* pnf = l.s_pnf;
    float* const* pnb = l.s_pnb;
    float* raypart = l.raypart;
    const RtIter first = iter(0);
    LidfQueryTrainArgs t;
    rt_query_args(q, l, first, &t);
    {   // every weight stream of the step — the forward launches' and the backward launches' — in one multi-pack
        JobScope js;
        if (chain)
            rc = pnetc_pack(q->pnet, l.s_pnchain, pnf, l.s_pnbwd, cus, st);
        else   // (pack only: no activation is touched)
            rc = pointnet_train_forward_impl(q->pnet, nullptr, nullptr, 0, 0, nullptr, first.pa, nullptr, pnf, cus, st, 1);
        if (!rc) {
            LidfPointNetGrads none = {};
            rc = pointnet_backward_impl(q->pnet, nullptr, nullptr, 0, 0, first.pa, nullptr, nullptr, &none, w.pw, false,
                                        pnb, 1, cus, st);
        }
        if (!rc)
            rc = qdec_forward_impl(&t, E, nullptr, nullptr, nullptr, nullptr, nullptr, l.s_vox, l.s_ray, l.s_chain, cus,
                                   st, 1);
        if (!rc) rc = rt_pack_transposed(dec, E, Ed, l.s_dvox, l.s_dpe, cus, st);
        if (!rc && flush_jobs(js.jobs, st) != hipSuccess) rc = LIDF_ERR_HIP;
        if (rc) return rc;
    }
    CHECK_HIP(lidf_launch_pack_dgrad(dec->w3, dec->w2, l.s_dgrad, st));
    CHECK_HIP(lidf_launch_iota(l.ray_idx, R, st));
    // the per-ray part of layer 1: the same in every iteration
    if ((rc = qdec_forward_impl(&t, E, nullptr, nullptr, raypart, nullptr, nullptr, nullptr, l.s_ray, nullptr, cus, st,
                                2, 2)))
        return rc;
    const float r0 = q->offset_range0, rs = q->offset_range1 - q->offset_range0;
    const float* cur = q->pred_pos;
    for (int it = 0; it < T; ++it) {
        const RtIter ib = iter(it);
        float* cur_keep = ib.cur;
        int* end_voxel = ib.end_voxel;
        // (the chains keep sorted copies of what their backward reads: one [valid | predicted] buffer serves every
        // iteration, its valid rows copied once per step; the layer-by-layer path keeps a buffer per iteration)
        float* pn_inp = chain ? first.pn_inp : ib.pn_inp;
        int* pn_vox = chain ? first.pn_vox : ib.pn_vox;
        float *pe = ib.pe, *off = ib.off;
        if (it == 0) {   // (later iterations start from the position the one before wrote into their block)
            CHECK_HIP(hipMemcpyAsync(cur_keep, cur, (size_t)R * 12, hipMemcpyDeviceToDevice, st));
            cur = cur_keep;
        }
        // final_pnet_inp = cat(valid points, predicted points), final_revidx likewise (pipeline.py:1007-1008)
        if (Nv > 0 && (!chain || it == 0)) {
            CHECK_HIP(hipMemcpyAsync(pn_inp, q->valid_inp, (size_t)Nv * 24, hipMemcpyDeviceToDevice, st));
            CHECK_HIP(hipMemcpyAsync(pn_vox, q->valid_vox, (size_t)Nv * 4, hipMemcpyDeviceToDevice, st));
        }
        cells.ready = q->cell_table_ready || it > 0;
        CHECK_HIP(lidf_launch_refine_prep(cur, (const long long*)q->max_pair_id, q->pair_vox, P, q->voxel_bound,
                                          q->voxel_bid, V, q->ray_bid, q->ray_flat, q->rgb_img,
                                          (long long)q->height * q->width, q->rayfeat, 128 + Ed, q->multires_views,
                                          q->multires, q->pnet_pos_rel, q->pos_rel, R, pn_inp + (size_t)Nv * 6,
                                          pn_vox + Nv, nullptr, 0, end_voxel, nullptr, st,
                                          q->voxel_coord ? &cells : nullptr));
        // the iteration's per-ray layer-1 rows [ROI | embed(pos [- centre]) | embed(dir)] in W1's column order
        // (columns 128 .. 128 + 206 of the reference's inp_embed; the kernel addresses a row as inp_embed + 128):
        // the chain reads its embed(pos) window, the backward's weight gradient all of it
        CHECK_HIP(lidf_launch_refine_rows_dev(cur, end_voxel, q->voxel_bound, q->rayfeat, 128 + Ed, q->multires_views,
                                              q->multires, q->pos_rel, R, nullptr, pe - 128, 128 + E + Ed, 0, st));
        if (chain)
            rc = pnetc_forward(pn_inp, pn_vox, n, V, nullptr, ib.pc, w.pcw, l.s_pnchain, pnf, cus, st);
        else
            rc = pointnet_train_forward_impl(q->pnet, pn_inp, pn_vox, n, V, ib.pa.out, ib.pa, w.pw.gpart, pnf, cus, st, 2);
        if (rc) return rc;
        rt_query_args(q, l, ib, &t);
        if ((rc = qdec_forward_impl(&t, E, off, ib.voxpart, raypart, ib.passes, ib.pre, l.s_vox, nullptr, l.s_chain,
                                    cus, st, 2, 1 | 4, 128 + E + Ed)))
            return rc;
        float* out = it == T - 1 ? q->pred_pos_out : iter(it + 1).cur;
        CHECK_HIP(lidf_launch_refine_finish(cur, off, q->ray_dir, r0, rs, R, out, st));
        if (it == T - 1 && q->end_voxel_id)
            CHECK_HIP(hipMemcpyAsync(q->end_voxel_id, end_voxel, (size_t)R * 4, hipMemcpyDeviceToDevice, st));
        cur = out;
    }
    return LIDF_OK;
}

LIDF_API int lidf_refine_train_backward_f32(const LidfRefineArgs* q, int32_t forward_times, const void* act_v,
                                              size_t act_bytes, const float* g_pos, float* d_pred_pos,
                                              float* d_rayfeat, const LidfPointNetGrads* gp,
                                              const LidfDecoderGrads* gd, lidf_stream_t stream) {
    int rc, cus;
    const int T = forward_times;
    if ((rc = rt_check(q, T, false))) return rc;   // (pred_pos_out / end_voxel_id are the forward's outputs)
    if (!gp || !gd) return LIDF_ERR_BAD_ARG;
    const LidfDecoder* dec = q->off;
    if (!gd->w1 || !gd->b1 || !gd->w2 || !gd->b2 || !gd->w3 || !gd->b3 || !gd->w4 || !gd->b4 ||
        (dec->is_ief && (!gd->wenc || !gd->benc)))
        return LIDF_ERR_BAD_ARG;
    if (!gp->w_p1 || !gp->b_p1 || !gp->w_p2 || !gp->b_p2 || !gp->w_v1 || !gp->b_v1 || !gp->w_p3 || !gp->b_p3 ||
        !gp->w_p4 || !gp->b_p4 || !gp->w_v2 || !gp->b_v2)
        return LIDF_ERR_BAD_ARG;
    const int64_t R = q->n_rays, Nv = q->n_valid, V = q->n_vox, n = R + Nv;
    const int E = 3 + 6 * q->multires, Ed = 3 + 6 * q->multires_views;
    const int D = refine_D(q->multires, q->multires_views), ld1 = D + (dec->is_ief ? 16 : 0);
    const int npass = dec->is_ief ? dec->n_iter : 1;
    hipStream_t st = (hipStream_t)stream;
    // the gradients start at zero (also what an empty batch returns)
    CHECK_HIP(zero_decoder_grads(gd, ld1, dec->is_ief, st));
    {
        float* const zp[12] = {gp->w_p1, gp->b_p1, gp->w_p2, gp->b_p2, gp->w_v1, gp->b_v1, gp->w_p3, gp->b_p3,
                               gp->w_p4, gp->b_p4, gp->w_v2, gp->b_v2};
        const long long zc[12] = {32 * 6, 32, 64 * 32, 64, 64 * 64, 64, 128 * 128, 128, 128 * 128, 128, 128 * 128, 128};
        CHECK_HIP(lidf_launch_zero_segments(zp, zc, 12, st));
    }
    if (R == 0) return LIDF_OK;
    if (!g_pos) return LIDF_ERR_BAD_ARG;
    Carver ca(act_v), cw(q->workspace);   // (the streams inside `act` are read, nothing of it is written)
    const RtLay l = rt_lay(ca, R, Nv, V, E, npass, T);
    const RtWs w = rt_ws(cw, R, Nv, V, E);
    CHECK_CARVED(ca, act_v, act_bytes);
    CHECK_CARVED(cw, q->workspace, q->workspace_bytes);
    if ((rc = cu_count(&cus))) return rc;
    const bool chain = pnetc_ok(n, V);
    float* const* pnb = l.s_pnb;
    float *ssum = w.ssum, *s_it = w.s_it, *dvoxfeat = w.dvoxfeat, *d_pe = w.d_pe, *d_inp = w.d_inp;
    const float rs = q->offset_range1 - q->offset_range0;
    const float* g = g_pos;
    for (int it = T - 1; it >= 0; --it) {
        Carver ci(l.iter0 + (size_t)it * l.iter_bytes);
        const RtIter ib = rt_iter(ci, R, Nv, V, E, npass);
        const float* cur = ib.cur;
        const int* end_voxel = ib.end_voxel;
        // does a gradient have to reach the position this iteration started from?
        const bool need_dcur = it > 0 || d_pred_pos != nullptr;
        // d off = rs <g, dir>, through the output activation: straight into the decoder backward's goff
        CHECK_HIP(lidf_launch_refine_train_goff(g, q->ray_dir, rs, R, ib.pre, dec->use_sigmoid, w.qw.goff, st));
        LidfQueryTrainArgs t;
        rt_query_args(q, l, ib, &t);
        QdecBwd o = {};
        o.E2 = E; o.zero_grads = false;
        // (the sum of S over the iterations is only needed for d_rayfeat; the last iteration's S opens it)
        o.S_keep = (d_rayfeat && it == T - 1) ? ssum : s_it;
        o.l1rows = ib.pe; o.l1_ld = 128 + E + Ed; o.l1_cols = 128 + E + Ed; o.l1_c0 = 128;
        o.d_pe = need_dcur ? d_pe : nullptr;
        o.s_dvox = l.s_dvox; o.s_dpe = l.s_dpe; o.pack_mode = 2;
        o.s_dgrad = l.s_dgrad;
        o.goff_ready = true;
        if (chain) {   // the PointNet's sort of this iteration groups the rays by end voxel already
            size_t sc_off, perm_off;
            int nblk;
            lidf_sort_idx_layout(n, V, &sc_off, &nblk, &perm_off);
            o.ss_perm = (const int*)(ib.pc.sort + perm_off);
            o.ss_vstart = ib.pc.vstart;
            o.ss_first = ib.pc.first;
            o.ss_row0 = Nv; o.ss_n = n;
            o.ss_partial = w.ss_partial;
        }
        if ((rc = qdec_backward_impl(&t, o, ib.passes, ib.pre, nullptr, dvoxfeat, nullptr, 0, gd, w.qw, cus, st)))
            return rc;
        if (d_rayfeat && it != T - 1) CHECK_HIP(lidf_launch_add_inplace(ssum, s_it, R * LIDF_H1, st));
        if (chain)
            rc = pnetc_backward(q->pnet, n, V, ib.pc, dvoxfeat, need_dcur ? d_inp : nullptr, true, gp, w.pcw, pnb, 2,
                                l.s_pnbwd, cus, st);
        else
            rc = pointnet_backward_impl(q->pnet, ib.pn_inp, ib.pn_vox, n, V, ib.pa, dvoxfeat,
                                        need_dcur ? d_inp : nullptr, gp, w.pw, false, pnb, 2, cus, st);
        if (rc) return rc;
        if (need_dcur) {
            float* gn = it == 0 ? d_pred_pos : w.g[it & 1];
            CHECK_HIP(lidf_launch_refine_train_dcur(g, cur, end_voxel, q->voxel_bound, q->pos_rel, d_pe, q->multires,
                                                    d_inp + (size_t)Nv * 6, R, gn, st));
            g = gn;
        }
    }
    // (dW1's ROI / embed(dir) columns came with every iteration's S^T [ROI | embed(pos) | embed(dir)] product)
    if (d_rayfeat) {   // raypart[r] = W1[:, 128:256] roi[r] + W1[:, 256 + E:] embed(dir)[r], on the sum of S
        float* sbuf = w.qw.stream;
        LinEx L = {};
        L.transposed = 1; L.ldw = ld1; L.k = LIDF_H1; L.ldx = LIDF_H1; L.X = ssum; L.n = R;
        L.w = dec->w1 + 128; L.nout = 128; L.out = d_rayfeat; L.ld_out = 128 + Ed;
        if ((rc = run_linex(L, sbuf, cus, st))) return rc;
        L.w = dec->w1 + 256 + E; L.nout = Ed; L.out = d_rayfeat + 128;
        if ((rc = run_linex(L, sbuf, cus, st))) return rc;
    }
    return LIDF_OK;
}

// ---- the per-ray step of one iteration as entries of their own (the any-width route, generic.refine_train) -------
// cells of a grid of `batch` frames: 0 = not a grid, -1 = more than the int32 table index holds
static long long rstep_n_cells(int32_t batch, const int32_t* grid_res) {
    if (!grid_res || batch <= 0) return 0;
    long long nc = batch;
    for (int k = 0; k < 3; ++k) {
        if (grid_res[k] <= 0) return 0;
        nc *= grid_res[k];
        if (nc > 0x7fffffffLL) return -1;
    }
    return nc;
}

LIDF_API size_t lidf_refine_step_workspace_bytes(int32_t batch, const int32_t* grid_res) {
    const long long nc = rstep_n_cells(batch, grid_res);
    return nc > 0 ? (size_t)nc * 4 : 0;
}

LIDF_API int lidf_refine_step_forward_f32(const float* pos, const int64_t* max_pair_id, const int32_t* pair_vox,
                                            int64_t n_pairs, const float* voxel_bound, const int32_t* voxel_bid,
                                            int64_t n_vox, const int32_t* ray_bid, const int32_t* ray_flat,
                                            const float* rgb_img, int32_t batch, int32_t height, int32_t width,
                                            int64_t n_rays, int64_t n_valid, int32_t pnet_pos_rel, int32_t pos_rel,
                                            int32_t multires, const int32_t* voxel_coord, const int32_t* grid_res,
                                            const float* grid_xmin, float grid_part, int32_t cell_table_ready,
                                            int32_t* end_voxel, float* pnet_inp, int32_t* pnet_vox, float* pe,
                                            int64_t ld_pe, void* workspace, size_t workspace_bytes,
                                            lidf_stream_t stream) {
    if (n_rays < 0 || n_pairs < 0 || n_vox < 0 || n_valid < 0 || multires < 0 || multires > 16)
        return LIDF_ERR_BAD_ARG;
    if (n_rays == 0) return LIDF_OK;
    if (n_vox == 0 || batch <= 0 || height <= 0 || width <= 0 || ld_pe < 3 + 6 * multires) return LIDF_ERR_BAD_ARG;
    if (!pos || !max_pair_id || !voxel_bound || !voxel_bid || !ray_bid || !ray_flat || !rgb_img || !end_voxel ||
        !pnet_inp || !pnet_vox || !pe || (n_pairs > 0 && !pair_vox))
        return LIDF_ERR_BAD_ARG;
    if (((uintptr_t)pos | (uintptr_t)pnet_inp | (uintptr_t)pe) & 3) return LIDF_ERR_BAD_ARG;
    if (n_rays + n_valid > 0x15555555LL || n_vox > 0x7fffffffLL || n_pairs > 0x7fffffffLL) return LIDF_ERR_UNSUPPORTED;
    CellLookup cells = {};
    if (voxel_coord) {   // the end voxels through the cell table, which lives in the workspace
        const long long nc = rstep_n_cells(batch, grid_res);
        if (nc == 0 || !grid_xmin || !(grid_part > 0.f)) return LIDF_ERR_BAD_ARG;
        if (nc < 0) return LIDF_ERR_UNSUPPORTED;
        CHECK_WS(workspace, workspace_bytes, (size_t)nc * 4);
        for (int k = 0; k < 3; ++k) {
            cells.g.xmin[k] = grid_xmin[k];
            cells.g.r[k] = grid_res[k];
        }
        cells.g.crop = grid_part;
        cells.g.B = batch;
        cells.coord = voxel_coord;
        cells.table = (int*)workspace;
        cells.ready = cell_table_ready;
    }
    RayStepArgs a = {};
    a.pos = pos; a.max_pair_id = (const long long*)max_pair_id; a.pair_vox = pair_vox;
    a.R = n_rays; a.P = n_pairs; a.V = n_vox; a.n_valid = n_valid;
    a.vbound = voxel_bound; a.vox_bid = voxel_bid; a.ray_bid = ray_bid; a.ray_flat = ray_flat;
    a.rgb = rgb_img; a.hw = (long long)height * width;
    a.pnet_rel = pnet_pos_rel ? 1 : 0; a.pos_rel = pos_rel ? 1 : 0; a.L = multires;
    a.end_voxel = end_voxel; a.pnet_inp = pnet_inp; a.pnet_vox = pnet_vox; a.pe = pe; a.ld_pe = ld_pe;
    CHECK_HIP(lidf_launch_refine_raystep(a, voxel_coord ? &cells : nullptr, (hipStream_t)stream));
    return LIDF_OK;
}

LIDF_API int lidf_refine_step_backward_f32(const float* g_pos, const float* ray_dir, float offset_range0,
                                             float offset_range1, float* d_off, const float* pos,
                                             const int32_t* end_voxel, const float* voxel_bound, int32_t pos_rel,
                                             const float* d_pe, int32_t multires, const float* d_pnet_rows,
                                             float* d_pos, int64_t n_rays, lidf_stream_t stream) {
    if (n_rays < 0 || multires < 0 || multires > 16) return LIDF_ERR_BAD_ARG;
    if (n_rays == 0 || (!d_off && !d_pos)) return LIDF_OK;
    if (!g_pos || (d_off && !ray_dir)) return LIDF_ERR_BAD_ARG;
    if (d_pos && d_pe && (!pos || (pos_rel && (!end_voxel || !voxel_bound)))) return LIDF_ERR_BAD_ARG;
    if (n_rays > 0x15555555LL) return LIDF_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    if (d_off)
        CHECK_HIP(lidf_launch_refine_train_goff(g_pos, ray_dir, offset_range1 - offset_range0, n_rays, nullptr, 0,
                                                d_off, st));
    if (d_pos)
        CHECK_HIP(lidf_launch_refine_train_dcur(g_pos, pos, end_voxel, voxel_bound, pos_rel ? 1 : 0, d_pe, multires,
                                                d_pnet_rows, n_rays, d_pos, st));
    return LIDF_OK;
}
