// lidf_launch.h — the host entry points of the kernel files: every launcher and size / layout helper that
// one .hip file defines and another file (lidf_api.hip and its .inc parts, or another kernel file) calls.
// Every .hip file includes this header, so each definition is compiled against the declaration its callers
// see: these are extern "C" names, matched by the linker by name alone, and a definition that disagrees
// with its declaration here is a compile error ("conflicting types") instead of a wrong launch.
// Grouped by defining file; parameter names are those of the definitions.
#pragma once
#include "lidf_device.h"

extern "C" {

// ---- lidf_points.hip
hipError_t lidf_launch_pack_multi(const PackJobs& j, hipStream_t st);
hipError_t lidf_launch_pack(const StreamLayout& lay, const NetW& n0, const NetW& n1, const L1Map& m, float* stream,
                            float* aux, hipStream_t st);
hipError_t lidf_launch_l1only_pair(const PointsArgs& a, const PointsArgs& b, const PointsArgs* c, int cus,
                                   hipStream_t st);
hipError_t lidf_launch_points(int mode, const PointsArgs& a, int grid, hipStream_t st);

// ---- lidf_points_h.hip
hipError_t lidf_launch_pack_h(const StreamLayout& lay, const NetW& n0, const NetW& n1, const L1Map& m, float* stream,
                              float* aux, hipStream_t st);
hipError_t lidf_launch_points_h(const PointsArgs& a, int cus, hipStream_t st);
hipError_t lidf_launch_points_h_list(const PointsArgs& a, int cus, hipStream_t st);

// ---- lidf_rows_h.hip
StreamLayout lidf_make_layout_rows_h(int nets, int D, int l1only);
hipError_t lidf_launch_pack_rows_h(const StreamLayout& lay, const NetW& n0, const NetW& n1, const L1Map& m,
                                   float* stream, float* aux, hipStream_t st);
hipError_t lidf_launch_rows_h(const PointsArgs& a, int grid, hipStream_t st);

// ---- lidf_linear.hip
hipError_t lidf_launch_vox2(const Vox2Args& a, hipStream_t st);
hipError_t lidf_launch_linear(int nt, const LinearArgs& a_in, int grid, hipStream_t st);

// ---- lidf_linear_s.hip, lidf_linear_x.hip, lidf_linear_sx.hip (one each; called by lidf_launch_linear)
void lidf_launch_linear_s(int nt, dim3 g, dim3 b, hipStream_t st, const LinearArgs& a);
void lidf_launch_linear_x(int nt, dim3 g, dim3 b, hipStream_t st, const LinearArgs& a);
void lidf_launch_linear_sx(int nt, dim3 g, dim3 b, hipStream_t st, const LinearArgs& a);

// ---- lidf_aux.hip
hipError_t lidf_launch_embed(const float* x, long long n, int L, float* out, hipStream_t st);
hipError_t lidf_launch_roi_align(const float* feat, int Cn, int H, int W, const int* ray_pix, const int* ray_bid,
                                 long long R, int half, int S, float* out, long long ld, hipStream_t st);
hipError_t lidf_launch_rayfeat(const float* feat, float* box, int B, int H, int W, const float* ray_dir,
                               const int* ray_pix, const int* ray_bid, long long R, int half, int Lv, float* out,
                               int ld, hipStream_t st);
hipError_t lidf_launch_rayfeat_phase(const float* feat, float* box, int B, int H, int W, const float* ray_dir,
                                     const int* ray_pix, const int* ray_bid, long long R, const int* R_dev, int half,
                                     int Lv, float* out, int ld, int phase, hipStream_t st);
hipError_t lidf_launch_rayfeat_dev(const float* feat, float* box, int B, int H, int W, const float* ray_dir,
                                   const int* ray_pix, const int* ray_bid, long long R, const int* R_dev, int half,
                                   int Lv, float* out, int ld, hipStream_t st);
hipError_t lidf_launch_zero_segments(float* const* ptrs, const long long* counts, int n, hipStream_t st);
// (the definition gives the five parameters behind the stream nullptr defaults, for lidf_launch_ray_reduce)
hipError_t lidf_launch_ray_reduce_dev(const float* prob, const float* pos, const int* off, long long R, long long P,
                                      const int* R_dev, const int* P_dev, const int* ray_bid, const int* ray_flat,
                                      long long hw, float* softmax, long long* maxid, float* pred_pos, float* depth,
                                      hipStream_t st, const int* pair_vox, const float* pair_t, int* sel_ray,
                                      int* sel_vox, float* sel_t);
hipError_t lidf_launch_selected_finish(const long long* maxid, const float* off_sel, const float* pos_sel,
                                       long long R, long long P, const int* R_dev, const int* P_dev,
                                       const int* ray_bid, const int* ray_flat, long long hw, float* pred_offset,
                                       float* pair_pred_pos, float* pred_pos, float* depth, hipStream_t st);
hipError_t lidf_launch_sel_from_ids(const long long* id, const int* pair_vox, const float* pair_t, long long R,
                                    long long P, int* sel_ray, int* sel_vox, float* sel_t, hipStream_t st);
hipError_t lidf_launch_ray_reduce(const float* prob, const float* pos, const int* off, long long R, long long P,
                                  const int* ray_bid, const int* ray_flat, long long hw, float* softmax,
                                  long long* maxid, float* pred_pos, float* depth, hipStream_t st);
hipError_t lidf_launch_ray_dirs(const float* intr, int B, int H, int W, float* dir, hipStream_t st);
hipError_t lidf_launch_ray_aabb_dense(const float* ray_dir, const float* vbound, const int* ray_bid,
                                      const int* vox_bid, long long R, long long V, int* mask, float* dist,
                                      hipStream_t st);
hipError_t lidf_launch_ray_aabb_compact(bool fill, const float* ray_dir, const float* vbound, const int* ray_bid,
                                        const int* vox_bid, long long R, long long V, int* count, const int* pair_off,
                                        int* pair_ray, int* pair_vox, float* pair_t, hipStream_t st);
size_t lidf_ray_aabb_onepass_lb_bytes(long long R_cap);
hipError_t lidf_launch_ray_aabb_onepass(const float* ray_dir, const float* vbound, const int* ray_bid,
                                        const int* vox_bid, long long R_cap, int* counts, void* lb, int* pair_off,
                                        int* pair_ray, int* pair_vox, float* pair_t, long long pair_cap,
                                        const int* vox_start, hipStream_t st);
hipError_t lidf_launch_ray_aabb_grid_build(const float* vbound, const int* vox_bid, const int* coord, long long V,
                                           int B, int rx, int ry, int rz, int* cell, unsigned* colmask, float* tab,
                                           hipStream_t st);
hipError_t lidf_launch_ray_aabb_grid(bool fill, const float* ray_dir, const int* ray_bid, long long R, int B, int rx,
                                     int ry, int rz, const int* cell, const unsigned* colmask, const float* tab,
                                     int* count, const int* pair_off, int* pair_ray, int* pair_vox, float* pair_t,
                                     hipStream_t st);
hipError_t lidf_launch_pcl_aabb_dense(const float* pos, const float* vbound, const int* pcl_bid, const int* vox_bid,
                                      long long N, long long V, int* mask, hipStream_t st);
hipError_t lidf_launch_pcl_aabb_last(const float* pos, const float* vbound, const int* pcl_bid, const int* vox_bid,
                                     long long N, long long V, int* last, hipStream_t st);
hipError_t lidf_launch_scan(const int* in, long long n, int* out, int* sums, hipStream_t st);
hipError_t lidf_launch_vox_mark(const float* xyz, const int* bid, long long N, const GridSpec& g, int* cell_flag,
                                int* pt_key, int* pt_valid, hipStream_t st);
hipError_t lidf_launch_vox_cells_bid(const int* cell_flag, const int* cell_rank, long long ncell, const GridSpec& g,
                                     int* occ, float* vbound, int* vox_bid, hipStream_t st);
hipError_t lidf_launch_vox_cells(const int* cell_flag, const int* cell_rank, long long ncell, const GridSpec& g,
                                 int* occ, float* vbound, hipStream_t st);
hipError_t lidf_launch_vox_points(const float* xyz, const int* pt_key, const int* pt_rank, const int* cell_rank,
                                  long long N, const GridSpec& g, int* pid, int* revidx, float* rel, hipStream_t st);
size_t lidf_depth_metrics_ws_bytes(void);
hipError_t lidf_launch_depth_metrics(const float* pred, const float* gt, const void* seg, int seg_dtype, int src_h,
                                     int src_w, int dst_h, int dst_w, float* out, void* ws, hipStream_t st);
hipError_t lidf_launch_depth_metrics_frames(const float* pred, const float* gt, const void* seg, int seg_dtype, int B,
                                            int src_h, int src_w, int dst_h, int dst_w, float* out, void* ws,
                                            hipStream_t st);
hipError_t lidf_launch_miss_block_count(const void* mask, int dtype, long long n, int* block_cnt, hipStream_t st);
hipError_t lidf_launch_miss_count(const void* mask, int dtype, long long n, int* block_cnt, int* block_off, int* sums,
                                  int* n_rays, hipStream_t st);
hipError_t lidf_launch_miss_fill(const void* mask, int dtype, long long n, const int* block_off, const float* intr,
                                 int H, int W, int* ray_bid, int* ray_flat, int* ray_pix, float* ray_dir,
                                 long long* bid64, long long* flat64, long long* pix64, hipStream_t st);
hipError_t lidf_launch_fingerprint(const float* const* ptrs, const long long* floats, int nseg,
                                   unsigned long long salt, LidfPackGuardState* guard, hipStream_t st);
hipError_t lidf_launch_fingerprint_multi(const float* const* ptrs, const long long* floats, const int* grp, int nseg,
                                         const unsigned long long* salts, int ngrp, void* guards, int guard_stride,
                                         hipStream_t st);

// ---- lidf_frame.hip
size_t lidf_frame_head_blocks(long long npix);
size_t lidf_frame_head_lb_bytes(long long npix);
hipError_t lidf_launch_frame_head(const float* valid_mask, const float* miss_mask, const float* xyz, const float* rgb,
                                  const float* intr, int B, int H, int W, int stride, const GridSpec& g, void* lb,
                                  int* counts, int* valid_bid, int* valid_flat, float* valid_xyz, float* valid_rgb,
                                  int* cell_flag, int* pt_key, int* pt_rank, int* ray_bid, int* ray_flat,
                                  int* ray_pix, float* ray_dir, float* depth, float* depth2, const int* idx_bid,
                                  const int* idx_flat, long long n_list, hipStream_t st);
hipError_t lidf_launch_frame_cells(const int* cell_flag, long long ncell, const GridSpec& g, int* cell_rank, int* occ,
                                   float* vbound, int* vox_bid, float* vox_center, int* counts, int* vox_start,
                                   hipStream_t st);
hipError_t lidf_launch_frame_points(const float* valid_xyz, const float* valid_rgb, const int* pt_key,
                                    const int* pt_rank, const int* cell_rank, const GridSpec& g, long long cap,
                                    const int* counts, int* pid, int* revidx, float* rel, float* pnet_inp,
                                    float* pnet_abs, hipStream_t st);
hipError_t lidf_launch_frame_select(const float* valid_mask, const int* ray_bid, const int* ray_flat, long long hw,
                                    long long R_cap, const int* counts, unsigned char* sel, hipStream_t st);

// ---- lidf_refine.hip
hipError_t lidf_launch_refine_step(const RefineStepArgs& a, long long R_cap, hipStream_t st);
hipError_t lidf_launch_refine_raystep(const RayStepArgs& a, const CellLookup* cells, hipStream_t st);
hipError_t lidf_launch_refine_prep(const float* pred_pos, const long long* max_pair_id, const int* pair_vox,
                                   long long P, const float* vbound, const int* vox_bid, long long V,
                                   const int* ray_bid, const int* ray_flat, const float* rgb, long long hw,
                                   const float* rayfeat, int ld_rf, int Lv, int L, int pnet_rel, int pos_rel,
                                   long long R, float* pnet_inp, int* pnet_vox, float* inp_embed, int ld_e,
                                   int* end_voxel, const unsigned char* pnet_select, hipStream_t st,
                                   const CellLookup* cells);
hipError_t lidf_launch_refine_prep_dev(const float* pred_pos, const long long* max_pair_id, const int* pair_vox,
                                       long long P, const float* vbound, const int* vox_bid, long long V,
                                       const int* ray_bid, const int* ray_flat, const float* rgb, long long hw,
                                       int pnet_rel, long long R, float* pnet_inp, int* pnet_vox, int* end_voxel,
                                       const unsigned char* pnet_select, const int* dims, const int* row0_dev,
                                       hipStream_t st, const CellLookup* cells);
hipError_t lidf_launch_refine_rows_dev(const float* pred_pos, const int* end_voxel, const float* vbound,
                                       const float* rayfeat, int ld_rf, int Lv, int L, int pos_rel, long long R,
                                       const int* R_dev, float* inp_embed, int ld_e, int pos_only, hipStream_t st);
hipError_t lidf_launch_refine_gather_dev(const float* vox_feat, const int* end_voxel, long long R, const int* R_dev,
                                         float* inp_embed, int ld_e, hipStream_t st);
hipError_t lidf_launch_refine_gather(const float* vox_feat, const int* end_voxel, long long R, float* inp_embed,
                                     int ld_e, hipStream_t st);
hipError_t lidf_launch_refine_finish(const float* pred_pos, const float* off, const float* ray_dir, float r0,
                                     float rs, long long R, float* out, hipStream_t st);
hipError_t lidf_launch_refine_finish_dev(const float* pred_pos, const float* off, const float* ray_dir, float r0,
                                         float rs, long long R, const int* R_dev, float* out, const int* ray_bid,
                                         const int* ray_flat, long long hw, float* depth, hipStream_t st);
hipError_t lidf_launch_refine_train_goff(const float* g, const float* dir, float rs, long long R, const float* pre,
                                         int use_sigmoid, float* goff, hipStream_t st);
hipError_t lidf_launch_refine_train_dcur(const float* g, const float* cur, const int* end_voxel, const float* vbound,
                                         int pos_rel, const float* d_pe, int L, const float* d_inp, long long R,
                                         float* out, hipStream_t st);
hipError_t lidf_launch_add_inplace(float* a, const float* b, long long n, hipStream_t st);
hipError_t lidf_launch_iota(int* p, long long n, hipStream_t st);

// ---- lidf_train.hip
hipError_t lidf_launch_wgrad(const float* A, long long lda, int M, const float* B, long long ldb, int N, long long n,
                             float* C, int ldc, float* db, float* g_wgrad_scratch, size_t g_wgrad_scratch_floats,
                             hipStream_t st);
hipError_t lidf_launch_out_act(const float* pre, long long n, int use_sigmoid, float* out, const float* g,
                               float* gpre, hipStream_t st);
hipError_t lidf_launch_l4_backward(const float* goff, const float* h3, const float* w4, float slope, long long n,
                                   float* dz3, float* dw4, float* db4, float* scratch, hipStream_t st);
hipError_t lidf_launch_ief_tail(const float* dz1, const float* off, const float* w1enc, int ld1, const float* wenc,
                                const float* benc, long long n, int s_mode, float* S, float* goff, float* dw1enc,
                                float* dwenc, float* dbenc, float* bacc, float* scratch, hipStream_t st);
hipError_t lidf_launch_ief_first_pass(const float* btot, float* bacc, float init, const float* w1enc, int ld1,
                                      const float* wenc, const float* benc, float* dw1enc, float* dwenc, float* dbenc,
                                      hipStream_t st);
hipError_t lidf_launch_build_rows(const int* pair_ray, const int* pair_vox, const float* pair_t, const float* ray_dir,
                                  const float* vox_center, int pos_rel, const float* vox_feat, const float* rayfeat,
                                  int ld_rf, int L, int Ed, long long P, float* rows, int D, hipStream_t st);
hipError_t lidf_launch_rows_backward(const float* d_rows, int D, int E2, const int* pair_off, const int* pair_vox,
                                     long long R, long long P, int Ed, float* d_vox_feat, float* d_rayfeat, int ld_rf,
                                     hipStream_t st);
hipError_t lidf_launch_rayfeat_backward(const float* d_rayfeat, int ld_rf, const int* ray_pix, const int* ray_bid,
                                        long long R, int half, int B, int H, int W, float* d_feat, float* gimg,
                                        int* aux, hipStream_t st);
hipError_t lidf_launch_rayfeat_backward_ordered(const float* d_rayfeat, int ld_rf, const int* ray_pix,
                                                const int* ray_bid, long long R, int half, int B, int H, int W,
                                                float* d_feat, float* gimg, int* aux, hipStream_t st);
hipError_t lidf_launch_pe_rows(const int* pair_ray, const int* pair_vox, const float* pair_t, const float* ray_dir,
                               const float* vox_center, int pos_rel, int L, long long P, float* pe, hipStream_t st,
                               const int* n_dev = nullptr, long long row0 = 0);
hipError_t lidf_launch_seg_sum_ray(const float* S, int F, const int* pair_off, long long R, float* out,
                                   hipStream_t st);
size_t lidf_seg_sum_idx_ws_bytes(long long P, long long V);
hipError_t lidf_launch_seg_sum_idx(const float* S, const int* idx, long long P, long long V, float* out, void* ws,
                                   size_t ws_bytes, hipStream_t st);
size_t lidf_sort_idx_ws_bytes(long long P, long long V);
void lidf_sort_idx_layout(long long P, long long V, size_t* scanned_off, int* nblk, size_t* perm_off);
hipError_t lidf_launch_sort_idx(const int* idx, long long P, const int* n_dev, long long V, void* ws,
                                const int** perm_out, const int** n_perm_out, hipStream_t st);
hipError_t lidf_launch_pair_pos(const float* off, const int* pair_ray, const float* pair_t, const float* ray_dir,
                                long long P, float r0, float rs, float sqrt3, float part, float* out, hipStream_t st,
                                const int* n_dev = nullptr);
hipError_t lidf_launch_ray_select(const float* pos, const long long* id, long long R, long long P, float* pred_pos,
                                  hipStream_t st);
hipError_t lidf_launch_pair_pos_backward(const float* g_pos, const float* g_pred, const long long* id,
                                         const int* pair_ray, const float* ray_dir, long long P, float k,
                                         float* d_off, hipStream_t st);
hipError_t lidf_launch_gather_sel_rows(const float* act, long long P, int npass, const long long* rows, long long R,
                                       const int* pair_vox, const float* pe, int E2, const float* g_pred,
                                       const float* g_extra, const float* ray_dir, float k, float* act_dst, int* pvox,
                                       float* pe_dst, float* g_dst, int* poff, hipStream_t st);
hipError_t lidf_launch_relu_mask(const float* g, const float* src, long long n, float* out, hipStream_t st);
hipError_t lidf_launch_segmax_arg(const float* f, const int* vox, const float* pool, long long N, int F, int* arg,
                                  hipStream_t st);
hipError_t lidf_launch_segmax_backward(const float* dp, const int* arg, const int* vox, const float* pool,
                                       long long N, int F, int accumulate, float* out, hipStream_t st);
hipError_t lidf_launch_seg_sum_rows(const float* S, const int* idx, long long N, int F, float* out, hipStream_t st);
hipError_t lidf_launch_embed_backward(const float* x, const float* g, long long n, int L, float* dx, hipStream_t st);

// ---- lidf_train_widths.hip
size_t lidf_roi_align_backward_ws_bytes(long long B, long long H, long long W);
hipError_t lidf_launch_roi_align_backward(const float* d_out, long long ld, const int* ray_pix, const int* ray_bid,
                                          long long R, int B, int Cn, int H, int W, int half, int S, float* d_feat,
                                          void* ws, hipStream_t st);
size_t lidf_seg_sum_idx_any_ws_bytes(long long n, long long V, int F);
hipError_t lidf_launch_seg_sum_idx_any(const float* S, int F, const int* idx, long long n, long long V, float* out,
                                       void* ws, size_t ws_bytes, hipStream_t st);

// ---- lidf_dgrad.hip
hipError_t lidf_launch_dgrad_chain(const float* w3, const float* w2, const float* dz3, const unsigned* m2,
                                   const unsigned* m1, long long n, float slope, float* dz2, float* dz1,
                                   int accumulate, float* stream, int cus, hipStream_t st);
size_t lidf_dgrad_stream_bytes(void);
hipError_t lidf_launch_pack_dgrad(const float* w3, const float* w2, float* stream, hipStream_t st);

// ---- lidf_pointnet.hip
hipError_t lidf_launch_pack_pointnet(const float* w_p1, const float* b_p1, const float* w_p2, const float* b_p2,
                                     const float* w_p3, const float* w_p4, const float* b_p4, float* stream,
                                     const LidfPackGuardState* guard, hipStream_t st);
size_t lidf_pointnet_chain_stream_bytes(void);
size_t lidf_pointnet_pool_scratch_bytes(long long V);
hipError_t lidf_launch_pointnet_chain(int stage, const float* stream, const float* inp, const int* vox,
                                      const float* gpart, float* pool, float* part, long long V, long long n, int cus,
                                      hipStream_t st);
hipError_t lidf_launch_pointnet_chain_dev(int stage, const float* stream, const float* inp, const int* vox,
                                          const float* gpart, float* pool, long long V_cap, int v_lds,
                                          long long n_cap, const int* n_dev, const int* V_dev, const int* perm,
                                          const int* n_perm, int cus, hipStream_t st);
int lidf_pointnet_lds_max_voxels(void);
size_t lidf_pointnet_sort_bytes(long long n, long long V);
size_t lidf_group_idx_bytes(long long n_cap, long long V);
hipError_t lidf_launch_group_idx(const int* vox, long long n_cap, const int* n_dev, long long V, void* ws,
                                 const int** perm_out, const int** n_perm_out, hipStream_t st);
hipError_t lidf_launch_pointnet_chain_sorted(int stage, const float* stream, const float* inp, const int* vox,
                                             const float* gpart, float* pool, long long V, long long n_cap,
                                             const int* perm, const int* n_perm, int cus, hipStream_t st);

// ---- lidf_pointnet_train.hip
hipError_t lidf_launch_pnet_train_fwd(int stage, const float* stream, const float* inp, const int* vox,
                                      const int* perm, const int* n_perm, const float* gpart, float* inps, int* voxs,
                                      float* f1s, float* f2s, float* f4s, void* pool64, long long V, long long n,
                                      int cus, hipStream_t st);
hipError_t lidf_launch_pnet_unpack(const void* pool64, long long count, float* pool, int* arg, hipStream_t st);
int lidf_pnet_chunk_rows(void);
hipError_t lidf_launch_pnet_tables(const int* scanned, int nblk, long long V, const int* n_perm, int* vstart,
                                   int* first, hipStream_t st);
hipError_t lidf_launch_pnet_bwd_a(const float* stream, const int* voxs, const int* n_perm, const float* dp2,
                                  const int* arg2, const float* f4s, float* dz4s, float* df2s, long long n, int cus,
                                  hipStream_t st);
hipError_t lidf_launch_pnet_bwd_b(const float* stream, const int* voxs, const int* perm, const int* n_perm,
                                  const float* df2s, const float* dp1, const int* arg1, const float* f2s,
                                  const float* f1s, float* dz2s, float* dz1s, float* d_inp, long long n, int cus,
                                  hipStream_t st);
hipError_t lidf_launch_pnet_dw4(const float* dp2, const int* arg2, const float* f4s, long long V, float* dW4,
                                float* db4, hipStream_t st);
hipError_t lidf_launch_pnet_segsum(const float* rows, const int* vstart, const int* first, long long V, long long n,
                                   float* partial, float* out, hipStream_t st);
hipError_t lidf_launch_pnet_gather_segsum(const float* S, const int* perm, long long row0, const int* vstart,
                                          const int* first, long long V, long long n, float* partial, float* out,
                                          hipStream_t st);

// ---- lidf_loss.hip
hipError_t lidf_launch_pair_labels(const float* xyz, const int* ray_bid, const int* ray_flat, long long hw,
                                   const int* pair_off, const int* pair_vox, const float* vbound, long long R,
                                   long long P, float* gt_pos, long long* label, float* labelf, long long* maxid,
                                   int* n_label, int* pix2ray, hipStream_t st);
size_t lidf_stage1_loss_partial_bytes(long long R);
hipError_t lidf_launch_stage1_loss(const LossArgs& a, float* gt_img, float* pred_img, hipStream_t st);
hipError_t lidf_launch_stage1_loss_backward(const LossArgs& a, hipStream_t st);
hipError_t lidf_launch_refine_loss(const LossArgs& a, float* pred_img, hipStream_t st);
hipError_t lidf_launch_refine_loss_backward(const LossArgs& a, hipStream_t st);
size_t lidf_eval_loss_partial_bytes(long long R);
hipError_t lidf_launch_eval_loss(const LossArgs& a, int pairs, hipStream_t st);
hipError_t lidf_launch_eval_depth_images(const LossArgs& a, const float* xyz_gt, float* pred_img, float* gt_img,
                                         hipStream_t st);
size_t lidf_eval_loss_frames_partial_bytes(int B, long long hw, int pairs);
hipError_t lidf_launch_eval_loss_frames(const LossArgs& a, int pairs, hipStream_t st);
hipError_t lidf_launch_eval_depth_images_frames(const LossArgs& a, const float* xyz_gt, float* pred_img,
                                                float* gt_img, hipStream_t st);

// ---- lidf_select.hip
size_t lidf_select_workspace_bytes(int n_jobs, long long n_max);
hipError_t lidf_launch_select(const SelectJob* jobs, int n_jobs, double ratio, const SelectCompose& c, void* ws,
                              hipStream_t st);

// ---- lidf_sample.hip
size_t lidf_sample_valid_masks_bytes(int B, int H, int W);
size_t lidf_sample_valid_ws_bytes(int B, int H, int W);
hipError_t lidf_launch_sample_valid(const void* mask, int dtype, int B, int H, int W, int n,
                                    const unsigned long long* rng, int* bid, int* flat, long long* idx,
                                    int* valid_cnt, void* ws, hipStream_t st);
hipError_t lidf_launch_miss_window(const void* mask, int dtype, const float* intr, int B, int H, int W, int n,
                                   const unsigned long long* rng, const int* starts, int* block_cnt, int* block_off,
                                   int* img_off, int* ray_bid, int* ray_flat, int* ray_pix, float* ray_dir,
                                   long long* bid64, long long* flat64, long long* pix64, int* window, int* n_rays,
                                   hipStream_t st);

// ---- lidf_chain16.hip
hipError_t lidf_launch_chain16(int gf, const Chain16Args& a, int cus, hipStream_t st);
// (the stage-2 decoder: gf 64, both tables and vox present, raypart row r for row r)
hipError_t lidf_launch_chain16_stage2(const Chain16Args& a, int cus, hipStream_t st);
hipError_t lidf_launch_chain16h(int gf, const Chain16Args& a, int cus, hipStream_t st);   // lidf_chain16_h.hip
hipError_t lidf_launch_chain16_bias_row(const float* b1, const float* w1enc, int ld1, const float* benc, int nout,
                                        float* out, hipStream_t st);
}  // extern "C"
