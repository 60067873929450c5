/*
 * regnet_hip.h -- C ABI of libregnet_hip.so: the MI355X (gfx950) replacement for the native part
 * of REGNet's PointNet++ hot path (the reference's CUDA extensions `pn2_ext` and `dgcnn_ext`).
 *
 * Conventions (all entry points):
 *   - plain device pointers + int64 sizes/element-strides, no torch types, no allocation, no
 *     global state that affects results (the only statics: a per-device "large-LDS attribute set" bit of the two
 *     row-chain kernels, a debugging environment switch read once); re-entrant; the caller owns every buffer (the
 *     Python binding allocates the outputs exactly like the reference does with at::zeros);
 *   - `stream` is a hipStream_t passed as void* (NULL = the legacy default stream, which is what
 *     the reference launches on);
 *   - return value: 0 on success, REGNET_ERR_* (<0) for an argument the reference would have
 *     rejected with TORCH_CHECK / CHECK_EQ / CHECK_GT / CHECK_GE, or a positive hipError_t from
 *     the launch (the reference's THCudaCheck(cudaGetLastError())).  Never throws.
 *   - float data is fp32 (the _f64 operators: double), indices are int64, xyz tensors are the reference's channel-first
 *     (B,3,N) views addressed through explicit element strides (sb, sc, sn), so the
 *     non-contiguous views ScoreNet passes (score_network.py:46, pointnet2.py:89-90) need no copy.
 *
 * Reference interface each function replaces is cited as file:line relative to
 * /root/reference/multi_model/utils/pn2_utils/.
 */
#ifndef REGNET_HIP_H_
#define REGNET_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define REGNET_OK 0
#define REGNET_ERR_SHAPE (-1)       /* CHECK_EQ / CHECK_GT / CHECK_GE style violation            */
#define REGNET_ERR_NULL (-2)        /* NULL pointer for a non-empty tensor                        */
#define REGNET_ERR_UNSUPPORTED (-3) /* size outside what this build supports (reported, not UB)  */

/* Library / build identification. */
int regnet_abi_version(void);
const char* regnet_build_info(void);
/* Human-readable text for a code returned by any entry point (static storage). */
const char* regnet_strerror(int code);

/* ---- pn2_ext.farthest_point_sample  (csrc/sampling.h:7-9, sampling_kernel.cu:126-170) --------
 * xyz (B,3,N) strided -> index (B,M) int64 contiguous.  index[b,0]=0; tie order is the
 * reference's (lane = j mod block, shared-memory tree).
 * Errors: M<=0 or N<M -> REGNET_ERR_SHAPE (CHECK_GT/CHECK_GE :136-137).                        */
int regnet_fps_f32(const float* xyz, int64_t sb, int64_t sc, int64_t sn, int64_t B, int64_t N,
                   int64_t M, int64_t* index, float* workspace, void* stream);
/* Scratch bytes regnet_fps_f32 needs for (B,N,M) -- regnet_fps_plan's [6], which says what they hold.  The callee
 * initialises them; `workspace` may be NULL when this returns 0.                                */
int64_t regnet_fps_workspace_bytes(int64_t B, int64_t N, int64_t M);
/* regnet_fps_f32 for a cloud that is itself a furthest-point-sampling sequence -- what PointNet++ does at levels 2 and 3:
 * FarthestPointSampler over the previous level's centroids in their pick order (pointnet2.py:40-42, modules.py:23-26).
 * Pick k+1 of the producing run was the furthest point of the WHOLE cloud from picks 0..k, hence also the furthest among
 * the picks themselves, with the same fp32 distance: sampling the sequence from index 0 re-derives 0, 1, 2, ... unless two
 * points TIE at a maximum (the reference's tie order depends on array positions, which differ between the two runs).
 *   first_tie (B) int32, may be NULL: written with the first pick position (>= 1) of THIS run whose choice was not a unique
 *             strict maximum (several holders, or all distances zero); 0x7fffffff when there was none; 0 = "not tracked"
 *             (the single-workgroup round kernels for short runs and the streaming kernels; cooperating workgroups count
 *             every pick of their exact one-pick path).
 *   prefix_ok (B) int32, may be NULL: the `first_tie` of the run that PRODUCED this cloud's order.  Scenes with
 *             prefix_ok[b] >= M get index[b, :] = 0 .. M-1 without sampling (and first_tie[b] = prefix_ok[b]); the others are
 *             sampled as by regnet_fps_f32.  Results are identical to regnet_fps_f32's either way.
 * Same workspace and errors as regnet_fps_f32.                                                                           */
int regnet_fps_chain_f32(const float* xyz, int64_t sb, int64_t sc, int64_t sn, int64_t B, int64_t N, int64_t M,
                         int64_t* index, float* workspace, const int32_t* prefix_ok, int32_t* first_tie, void* stream);
/* Byte offset, inside that workspace, of the launch's 32-bit status word, or -1 when the kernel (B,N,M) selects has
 * none (every single-workgroup kernel).  The cooperative kernels (N > 25600) poll each other's exchange slots with a
 * bounded budget; a workgroup whose partner never answered ORs bit 0 into the word and stops sampling -- `index` is
 * then incomplete.  The callee zeroes the word; the caller reads it once the stream has passed the launch (the Python
 * binding accumulates it into a per-device flag and raises lazily: pn2_ext.raise_if_fps_failed).                      */
int64_t regnet_fps_status_offset_bytes(int64_t B, int64_t N, int64_t M);
/* regnet_fps_plan: HOST code, no device and no stream -- which kernel, grid and workspace regnet_fps_f32 and
 * regnet_fps_chain_f32 take for these sizes (the launcher and the two queries above call the same function; the only input
 * besides the sizes is the device's compute-unit count, 256 where there is no device).  plan (9 int64, host memory):
 *   [0] kernel family: 1 fps_resident_kernel (points in registers, one pick per round), 2 fps_cluster_kernel (Morton-sorted,
 *       pruning per 64-point cluster, several picks per round), 3 fps_sorted_kernel (sorted, pruning per wave), 4
 *       fps_cluster_kernel on cooperating workgroups, 5 fps_multi_kernel (cooperating workgroups, one pick per round),
 *       6 fps_streaming_kernel (running distances in the workspace); 0: nothing is launched (B == 0);
 *   [1] threads per workgroup, [2] points per thread (0 for family 6);
 *   [3] workgroups per scene G, [4] scenes padded to a multiple of 8 when G > 1 (else B), [5] grid = [3] * [4] workgroups;
 *   [6] workspace bytes: B*N*4 for family 2 (the sort's permutation); families 4-6 are all sized B*N*4 (the permutation /
 *       the running distances; family 5 leaves these words unused), rounded up to 16, + 16640 bytes of exchange area per
 *       scene + 256 bytes for the status word;
 *   [7] byte offset of the exchange area in the workspace (family 5 keeps its 64 bytes per scene at offset 0), -1: none;
 *   [8] byte offset of the status word = regnet_fps_status_offset_bytes, -1: none (every family but 4).
 * Returns what regnet_fps_f32 returns for these sizes before it looks at a pointer (REGNET_ERR_SHAPE, or REGNET_ERR_UNSUPPORTED
 * for N >= 2^30: plan zeroed); B == 0: success, [0]-[6] zero, [7] = [8] = -1; plan == NULL -> REGNET_ERR_NULL.                 */
int regnet_fps_plan(int64_t B, int64_t N, int64_t M, int64_t* plan);

/* ---- pn2_ext.ball_query  (csrc/ball_query.h:7-11, ball_query_kernel.cu:87-131) ---------------
 * xyz (B,3,N1) strided, centroids (B,3,N2) strided -> index (B,N2,K) int64, count (B,N2) int64.
 * First K points in index order with d2 < radius*radius (fp32, strict); first hit pre-fills all
 * K slots; a ball with no hit keeps index 0 / count 0 (the reference's at::zeros).              */
int regnet_ball_query_f32(const float* xyz, int64_t sb, int64_t sc, int64_t sn,
                          const float* centroids, int64_t cb, int64_t cc, int64_t cn, int64_t B,
                          int64_t N1, int64_t N2, float radius, int64_t K, int64_t* index,
                          int64_t* count, void* stream);

/* ---- uniform-grid variants of the two all-pairs scans (same results, fewer distance evaluations) ----
 * The source points (keys of the 3-NN search / the cloud of the ball query) are binned into cubic cells
 * inside a caller-provided workspace of regnet_grid_workspace_bytes(B, N_source) bytes (16-byte aligned);
 * outputs are bit-identical to regnet_three_nn_f32 / regnet_ball_query_f32.  The ball-query variant
 * supports K <= 64 (REGNET_ERR_UNSUPPORTED otherwise: use the plain entry point).                    */
int64_t regnet_grid_workspace_bytes(int64_t B, int64_t N_source);
int regnet_three_nn_grid_f32(const float* query, int64_t qb, int64_t qc, int64_t qn, const float* key,
                             int64_t kb, int64_t kc, int64_t kn, int64_t B, int64_t N1, int64_t N2,
                             int64_t* index, float* dist2, void* workspace, void* stream);
int regnet_ball_query_grid_f32(const float* xyz, int64_t sb, int64_t sc, int64_t sn,
                               const float* centroids, int64_t cb, int64_t cc, int64_t cn, int64_t B,
                               int64_t N1, int64_t N2, float radius, int64_t K, int64_t* index,
                               int64_t* count, void* workspace, void* stream);

/* ---- pn2_ext.group_points_forward / backward  (csrc/grouping.h:7-14) ------------------------
 * forward : input (B,C,N1) strided, index (B,N2,K) contiguous -> out (B,C,N2,K) contiguous.
 * backward: grad_out (B,C,N2,K) strided -> grad_in (B,C,N1) contiguous, zero-filled by callee. */
int regnet_group_points_fwd_f32(const float* input, int64_t sb, int64_t sc, int64_t sn,
                                const int64_t* index, int64_t B, int64_t C, int64_t N1, int64_t N2,
                                int64_t K, float* out, void* stream);
int regnet_group_points_bwd_f32(const float* grad_out, int64_t sb, int64_t sc, int64_t sn2,
                                int64_t sk, const int64_t* index, int64_t B, int64_t C, int64_t N1,
                                int64_t N2, int64_t K, float* grad_in, void* stream);

/* ---- pn2_ext.point_search (3-NN)  (csrc/interpolate.h:8-11, interpolate_kernel.cu:88-128) ----
 * query (B,3,N1), key (B,3,N2) strided -> index (B,N1,3) int64, dist2 (B,N1,3) fp32 ascending
 * SQUARED distances, earlier key wins ties.  N2<3 -> REGNET_ERR_SHAPE (CHECK_GE :102).          */
int regnet_three_nn_f32(const float* query, int64_t qb, int64_t qc, int64_t qn, const float* key,
                        int64_t kb, int64_t kc, int64_t kn, int64_t B, int64_t N1, int64_t N2,
                        int64_t* index, float* dist2, void* stream);

/* ---- pn2_ext.interpolate_forward / backward  (csrc/interpolate.h:13-22) ----------------------
 * forward : input (B,C,M) strided, index/weight (B,N,3) contiguous -> out (B,C,N) contiguous.
 * backward: grad_out (B,C,N) strided -> grad_in (B,C,M) contiguous, zero-filled by callee.      */
int regnet_interpolate_fwd_f32(const float* input, int64_t sb, int64_t sc, int64_t sm,
                               const int64_t* index, const float* weight, int64_t B, int64_t C,
                               int64_t M, int64_t N, float* out, void* stream);
int regnet_interpolate_bwd_f32(const float* grad_out, int64_t sb, int64_t sc, int64_t sn,
                               const int64_t* index, const float* weight, int64_t B, int64_t C,
                               int64_t M, int64_t N, float* grad_in, void* stream);

/* ---- dgcnn_ext.gather_knn_forward / backward  (functions/csrc/gather_knn.h) ------------------
 * Same gather / scatter-add as group_points with N2 == number of index rows.                    */
int regnet_gather_knn_fwd_f32(const float* input, int64_t sb, int64_t sc, int64_t sn,
                              const int64_t* index, int64_t B, int64_t C, int64_t N, int64_t NI,
                              int64_t K, float* out, void* stream);
int regnet_gather_knn_bwd_f32(const float* grad_out, int64_t sb, int64_t sc, int64_t sn2,
                              int64_t sk, const int64_t* index, int64_t B, int64_t C, int64_t N,
                              int64_t NI, int64_t K, float* grad_in, void* stream);

/* ---- float64 operators (csrc/ops_f64.hip, backwards in csrc/scatter.hip) ------------------------------------------------
 * The reference dispatches every pn2_ext / dgcnn_ext kernel on float32 and float64 (AT_DISPATCH_FLOATING_TYPES).  These
 * are the float64 instances: same arguments and semantics as the _f32 entry points above, with double data (indices stay
 * int64), plus caller-provided scratch where noted.  Nothing here is reached by float32 data.
 *   - distances are ((dx*dx) + (dy*dy)) + (dz*dz) in individually rounded double operations;
 *   - regnet_fps_f64: the reference's tie order for its block of get_block(N) (min 16) threads, as regnet_fps_f32;
 *     workspace of regnet_fps_f64_workspace_bytes(B, N, M) bytes (the running distances, initialised by the callee);
 *   - regnet_ball_query_f64: `radius` is a float as in the reference (ball_query_kernel.cu:90): widened to double and
 *     squared in double; strict d2 < r2;
 *   - regnet_three_nn_f64: dist2 in double; the reference's initial {1e40, 0, 0} / {-1, 0, 0} state as it is;
 *   - interpolate forward: ((+0 + x0*w0) + x1*w1) + x2*w2; weight (B,N,3) double, contiguous;
 *   - the three backwards are deterministic: grad_in[b,c,n] = the sum of the contributions to n in ascending flattened
 *     source position (group / gather_knn: m*K + k; interpolate: n*3 + k, adding the rounded product g*w), from +0.0 --
 *     the bits of numpy's np.add.at.  grad_in is written whole (no zero fill needed).  Workspace of
 *     regnet_scatter_f64_workspace_bytes(B, num_dest, num_src) bytes, 16-byte aligned (group / gather_knn: num_dest = N1
 *     or N, num_src = N2*K or NI*K; interpolate: num_dest = M, num_src = N*3).  Source indices outside [0, num_dest)
 *     contribute nothing; forward gathers read them as 0.                                                                 */
int64_t regnet_fps_f64_workspace_bytes(int64_t B, int64_t N, int64_t M);
int regnet_fps_f64(const double* xyz, int64_t sb, int64_t sc, int64_t sn, int64_t B, int64_t N, int64_t M,
                   int64_t* index, double* workspace, void* stream);
int regnet_ball_query_f64(const double* xyz, int64_t sb, int64_t sc, int64_t sn, const double* centroids, int64_t cb,
                          int64_t cc, int64_t cn, int64_t B, int64_t N1, int64_t N2, float radius, int64_t K,
                          int64_t* index, int64_t* count, void* stream);
int regnet_three_nn_f64(const double* query, int64_t qb, int64_t qc, int64_t qn, const double* key, int64_t kb,
                        int64_t kc, int64_t kn, int64_t B, int64_t N1, int64_t N2, int64_t* index, double* dist2,
                        void* stream);
int64_t regnet_scatter_f64_workspace_bytes(int64_t B, int64_t num_dest, int64_t num_src);
int regnet_group_points_fwd_f64(const double* input, int64_t sb, int64_t sc, int64_t sn, const int64_t* index, int64_t B,
                                int64_t C, int64_t N1, int64_t N2, int64_t K, double* out, void* stream);
int regnet_group_points_bwd_f64(const double* grad_out, int64_t sb, int64_t sc, int64_t sn2, int64_t sk,
                                const int64_t* index, int64_t B, int64_t C, int64_t N1, int64_t N2, int64_t K,
                                double* grad_in, void* workspace, void* stream);
int regnet_interpolate_fwd_f64(const double* input, int64_t sb, int64_t sc, int64_t sm, const int64_t* index,
                               const double* weight, int64_t B, int64_t C, int64_t M, int64_t N, double* out,
                               void* stream);
int regnet_interpolate_bwd_f64(const double* grad_out, int64_t sb, int64_t sc, int64_t sn, const int64_t* index,
                               const double* weight, int64_t B, int64_t C, int64_t M, int64_t N, double* grad_in,
                               void* workspace, void* stream);
int regnet_gather_knn_fwd_f64(const double* input, int64_t sb, int64_t sc, int64_t sn, const int64_t* index, int64_t B,
                              int64_t C, int64_t N, int64_t NI, int64_t K, double* out, void* stream);
int regnet_gather_knn_bwd_f64(const double* grad_out, int64_t sb, int64_t sc, int64_t sn2, int64_t sk,
                              const int64_t* index, int64_t B, int64_t C, int64_t N, int64_t NI, int64_t K,
                              double* grad_in, void* workspace, void* stream);

/* ---- region grouping (host Python loops in the reference) -----------------------------------
 * regnet_radius_group_f32: dataset_utils/get_regiondataset.py:279-295,:311-352.
 * pc (B,N,*) rows with xyz first (strides pb,pn in floats), centres (B,NC,*) likewise ->
 * cand (B,NC,cap) int32 = ascending indices of the points with d2 <= d2_threshold (inclusive),
 * count (B,NC) int32 = number of members (may exceed cap; only the first cap are stored).
 * The caller derives d2_threshold from the reference's `sqrt(d2) <= R` test (see
 * region_ops.sqrt_le_threshold).                                                                 */
int regnet_radius_group_f32(const float* pc, int64_t pb, int64_t pn, const float* centres,
                            int64_t cb, int64_t cn, int64_t B, int64_t N, int64_t NC,
                            float d2_threshold, int64_t cap, int32_t* cand, int32_t* count,
                            void* stream);

/* regnet_select_positive_f32: dataset_utils/get_regiondataset.py:354-434 (the `score > thr` mask +
 * torch.nonzero per scene of the centre picker).  pc (B,N,*) rows with xyz first (strides pb,pn),
 * score (B,N) (row stride sb) -> index (B,N) int64: first count[b] entries = ascending ids of the
 * points with score > threshold (strict); xyz_out (B,3,N) contiguous: their coordinates in that
 * order, slots >= count[b] repeat the first positive; count (B) int32.                          */
int regnet_select_positive_f32(const float* pc, int64_t pb, int64_t pn, const float* score, int64_t sb,
                               int64_t B, int64_t N, float threshold, int64_t* index, float* xyz_out,
                               int32_t* count, void* stream);

/* regnet_box_crop_f32: multi_model/gripper_region_network.py:508-544 (the per-grasp torch.nonzero
 * loop).  group_points (n,G,*) rows with xyz first (strides gb,gn), centre (n,3), rot (n,3,3)
 * row-major = [approach; axis_y; minor_normal], xlim/ylim (n) per-grasp half extents, zlim
 * scalar -> cand (n,G) int32 ascending in-box positions, count (n) int32.                       */
int regnet_box_crop_f32(const float* group_points, int64_t gb, int64_t gn, const float* centre,
                        const float* rot, const float* xlim, const float* ylim, float zlim,
                        int64_t n, int64_t G, int32_t* cand, int32_t* count, void* stream);

/* regnet_gather_max_f32: multi_model/gripper_region_network.py:388-395 + utils/pointnet2.py:167
 * (and :334-343 + pointnet2.py:232 for the refine stage): out[r,:] = max_g feat[rows[r,g],:].
 * feat (num_rows,F) row-major, rows (R,G) int64 -> out (R,F).                                    */
int regnet_gather_max_f32(const float* feat, int64_t num_rows, int64_t F, const int64_t* rows,
                          int64_t R, int64_t G, float* out, void* stream);
/* regnet_gather_max_scene_f32: the same with the reference's `index + b * N` (gripper_region_network.py:388, :334) formed in
 * the address: output row r pools the index list rows[rid], rid = row_ids ? row_ids[r] : r (int64 device, R entries), whose
 * entries are LOCAL point ids of scene rid / per_scene; global feature row = entry + (rid / per_scene) * scene_stride.
 * Negative entries are skipped.  Needs F % 4 == 0 and a 16-byte aligned feat (REGNET_ERR_UNSUPPORTED otherwise).          */
int regnet_gather_max_scene_f32(const float* feat, int64_t num_rows, int64_t F, const int64_t* rows, const int64_t* row_ids,
                                int64_t R, int64_t G, int64_t per_scene, int64_t scene_stride, float* out, void* stream);

/* ---- per-point shared-MLP contraction on fp32 MFMA (channels-last activations) ---------------
 * Replaces the cuDNN/cuBLAS 1x1-conv + BatchNorm + ReLU chains the reference runs for
 * SharedMLP (pn2_utils/nn/modules/mlp.py:55-114, conv.py:6-76) inside PointNetSAModule.forward
 * (pn2_utils/modules.py:210-246), PointnetFPModule.forward (:500-509) and the head
 * (utils/pointnet2.py:116-119).  W is packed [Npad][Kpad] (Npad multiple of 128, Kpad multiple of
 * 16, zero padded); scale/shift are the eval-mode BatchNorm folded to a per-channel affine.
 *
 * regnet_mlp_layer_f32: C[P,N] = act(scale * (A[P,Ka] . W^T) + shift); pool_group == 64 additionally
 * takes the max over every 64 consecutive rows (torch.max(x, 3), modules.py:245) -> C[P/64, N].
 *
 * What is read and written (all entry points of this section and regnet_sa_premul_layer_f32, regnet_interp_concat_f32,
 * regnet_interp_affine_f32, regnet_score_head_f32 below; tests/test_gpu_mlp_modes.py): an operand with a leading
 * dimension of its own is read in its valid columns only -- A below Ka, feat below Cf, U and V below C1, Yd and the
 * output's scale / shift below C, x below C -- so the padding up to lda / ldu / ldv / ldd / ldx may hold anything, NaN
 * included; the zero columns of the operand up to Kpad come from the kernel, not from memory.  Index arrays are read
 * for the rows of the problem only.  Of the output exactly the rows below P (P / 64 when pooled) and the columns below
 * N (Cout, C) are written: columns [N, ldc) and whatever follows the last row are left as they were, for any P, N and
 * ldc, aligned or not.                                                                                              */
int regnet_mlp_layer_f32(const float* A, int64_t lda, int64_t Ka, const float* W, int64_t Kpad,
                         const float* scale, const float* shift, float* C, int64_t ldc, int64_t P,
                         int64_t N, int relu, int pool_group, void* stream);

/* regnet_mlp_layer_splitk_f32: regnet_mlp_layer_f32 (no pooling) for SKINNY problems -- few rows, long K, e.g. the
 * grasp-region heads on B*64 regions (pointnet2.py:165-197, :227-254), where a 128-row tile grid cannot fill the
 * chip.  The K range is cut into `ksplit` slices multiplied by different workgroups; the slices' raw partial sums go
 * to `workspace` (regnet_mlp_splitk_workspace_bytes(P, N, ksplit) bytes, 16-byte aligned) and a second kernel adds
 * them IN INDEX ORDER and applies the affine + ReLU, so the result is deterministic.  1 <= ksplit <= Kpad / 16.   */
int64_t regnet_mlp_splitk_workspace_bytes(int64_t P, int64_t N, int64_t ksplit);
int regnet_mlp_layer_splitk_f32(const float* A, int64_t lda, int64_t Ka, const float* W, int64_t Kpad,
                                const float* scale, const float* shift, float* C, int64_t ldc, int64_t P,
                                int64_t N, int relu, int64_t ksplit, void* workspace, void* stream);

/* regnet_mlp_layer_plan: HOST code, no device and no stream -- which kernel and grid regnet_mlp_layer_f32 takes for these
 * sizes (the launcher calls the same function, environment switches included).  plan (8 int64, host memory):
 *   [0] tile rows, [1] tile columns, [2] waves per workgroup, [3] workgroups per CU -- all 0 for the two-buffer kernel of
 *       mlp.hip (mlp_gemm_kernel, taken when Kpad == 16: fewer than the two k-tiles the LDS-DMA ring starts with);
 *   [4] k-tiles (of 16 columns) per accumulation slab, 0 = one chain over all of K;
 *   [5] workgroups that compute one full tile each, [6] tiles of the last partial round that are cut into row slices
 *       (tail split), [7] slices per such tile (2), 0 when [6] is 0.  The grid is [5] + [6] * [7] workgroups.
 * Returns what regnet_mlp_layer_f32 returns for these sizes (REGNET_ERR_SHAPE / REGNET_ERR_UNSUPPORTED, plan zeroed);
 * P == 0: success, plan zeroed; plan == NULL -> REGNET_ERR_NULL.                                                        */
int regnet_mlp_layer_plan(int64_t P, int64_t N, int64_t Kpad, int pool_group, int64_t* plan);

/* regnet_sa_layer1_f32: first SharedMLP layer of a set-abstraction block with the grouping fused
 * into the operand load (no (B,C,M,K) tensor is materialised; reference: QueryGrouper.forward,
 * modules.py:39-56).  Row p = (b, m, k): A[p] = [feat[b, nbr[p], 0:Cf] | xyz[b,:,nbr[p]] -
 * xyz[b,:,ctr[b*M+m]]]; W columns must be packed in that order (features first).  feat element
 * (b,n,c) at feat[b*fb + n*fn + c*fc]; xyz (B,3,N) with strides (xb,xc,xn); nbr (B,M,group) int64,
 * ctr (B,M) int64.  -> C[B*M*group, N].                                                          */
int regnet_sa_layer1_f32(const float* feat, int64_t fb, int64_t fn, int64_t fc, int64_t Cf,
                         const float* xyz, int64_t xb, int64_t xc, int64_t xn, const int64_t* nbr,
                         const int64_t* ctr, int64_t B, int64_t M, int64_t group, const float* W,
                         int64_t Kpad, const float* scale, const float* shift, float* C, int64_t ldc,
                         int64_t N, int relu, void* stream);

/* regnet_sa_layer12_f32: like regnet_sa_layer1_f32 but with the FIRST TWO SharedMLP layers of the block in
 * one kernel, for blocks whose gathered input is narrow (Cf + 3 <= 8, i.e. the level-1 SA of ScoreNet:
 * 3 rgb + 3 xyz).  Layer 1 (W1 packed [C1][8] with columns [feat | xyz | 0], folded BN scale1/shift1,
 * ReLU) runs on the VALU inside the operand load of layer 2 (W packed [Npad][Kpad = C1]); the (P x C1)
 * layer-1 activation never reaches HBM.  pool_group as in regnet_mlp_layer_f32.                      */
int regnet_sa_layer12_f32(const float* feat, int64_t fb, int64_t fn, int64_t fc, int64_t Cf,
                          const float* xyz, int64_t xb, int64_t xc, int64_t xn, const int64_t* nbr,
                          const int64_t* ctr, int64_t B, int64_t M, int64_t group, const float* W1,
                          const float* scale1, const float* shift1, int64_t C1, const float* W,
                          int64_t Kpad, const float* scale, const float* shift, float* C, int64_t ldc,
                          int64_t N, int relu, int pool_group, void* stream);

/* regnet_sa_chain3_f32: a WHOLE narrow-input set-abstraction block in one kernel (pn2_utils/modules.py:210-246
 * for the level-1 block of PointNet2Seg, pointnet2.py:40-42): gather [feat | xyz - centre] (Cf + 3 <= 8) ->
 * layer 1 (W1 [C1][8], VALU) -> layer 2 (W2 packed [128][K2pad = 128]) -> layer 3 (W3 packed [C3pad][K3pad = 128],
 * C3 % 32 == 0) -> max over the group's 64 neighbours -> out (B*M, ldo).  Layers 1 and 2 always apply their folded
 * BN affine + ReLU, layer 3 its affine and ReLU if relu3.  The products are formed transposed (channels x points)
 * so each layer's MFMA accumulator is the next layer's B operand: no activation is written to LDS or HBM.
 * `count` (B*M int64, optional): the ball query's member counts -- slots >= count of a neighbourhood repeat slot 0
 * (regnet_ball_query_f32), so a neighbourhood with <= 32 members needs only its first 32 slots and half the MFMAs,
 * and two neighbourhoods with 33..48 members that sit 4 apart in a workgroup's 8 (slots 8 g + w and 8 g + w + 4 of
 * the processing order) share their third 32-row tile: three tiles of MFMAs for the pair instead of four.
 * `order` (B*M int64, optional): a permutation of the neighbourhoods giving the order in which workgroups (8
 * neighbourhoods each) take them; sorting by member-count class (<= 32, 33..48, more) makes whole workgroups of
 * one kind.  Outputs do not depend on `count` / `order` (bit-identical with and without).
 * Supported: group == 64, C1 == C2 == 128; anything else returns REGNET_ERR_UNSUPPORTED (use the layer-wise
 * entry points).  Same values as regnet_sa_layer12_f32 + regnet_mlp_layer_f32(pool) up to fp32 summation order. */
int regnet_sa_chain3_f32(const float* feat, int64_t fb, int64_t fn, int64_t fc, int64_t Cf, const float* xyz,
                         int64_t xb, int64_t xc, int64_t xn, const int64_t* nbr, const int64_t* ctr,
                         const int64_t* count, const int64_t* order, int64_t B, int64_t M, int64_t group,
                         const float* W1, const float* scale1,
                         const float* shift1, int64_t C1, const float* W2, int64_t K2pad,
                         const float* scale2, const float* shift2, int64_t C2, const float* W3,
                         int64_t K3pad, const float* scale3, const float* shift3, int64_t C3, int relu3,
                         float* out, int64_t ldo, void* stream);

/* regnet_pack_rows_f32: channels-last rows [feature(Cf) | xyz(3) | 0...] (width W >= Cf + 3) of all B*N source points,
 * the operand of the per-source-point first layer (U, V of regnet_sa_premul_layer_f32); feat (B,Cf,N) and xyz (B,3,N)
 * with element strides (b, c, n).  Replaces a zero fill and two strided copies.                                    */
int regnet_pack_rows_f32(const float* feat, int64_t fb, int64_t fc, int64_t fn, int64_t Cf, const float* xyz,
                         int64_t xb, int64_t xc, int64_t xn, int64_t B, int64_t N, int64_t W, float* out,
                         void* stream);
/* regnet_pack_rows_centred_f32: the same with the xyz columns written as xyz - mu[b] (mu (B,3) contiguous device floats, or
 * NULL = regnet_pack_rows_f32): the scene-mean centring of the pre-multiplied first layer (fused.PREMUL_CENTRE) inside the
 * pack instead of as a tensor subtraction in front of it -- one fp32 subtraction per value either way, same bits.          */
int regnet_pack_rows_centred_f32(const float* feat, int64_t fb, int64_t fc, int64_t fn, int64_t Cf, const float* xyz,
                                 int64_t xb, int64_t xc, int64_t xn, const float* mu, int64_t B, int64_t N, int64_t W,
                                 float* out, void* stream);

/* ---- gather_points (multi_model/utils/pn2_utils/function.py:11-26; callers modules.py:41, :238) ---------------------
 * out[b][c][m] = points[b][c][index[b][m]]: points element (b,c,n) at points[b*pb + c*pc + n*pn], index (b,m) at
 * index[b*ib + m*im] (int64), out element (b,c,m) at out[b*ob + c*oc + m*om].  An index outside [0, N) writes 0 and ORs 1
 * into *status (device int32, may be NULL) -- torch.gather raises for it; the Python wrapper checks lazily.                  */
int regnet_gather_points_f32(const float* points, int64_t pb, int64_t pc, int64_t pn, int64_t B, int64_t C, int64_t N,
                             const int64_t* index, int64_t ib, int64_t im, int64_t M, float* out, int64_t ob, int64_t oc,
                             int64_t om, int32_t* status, void* stream);

/* regnet_class_order_i64: order (n) int64 = the stable sort permutation of the level-1 neighbourhoods by cost class
 * (count > 32) + (count > 48) -- what torch.argsort(class, stable=True) returns (fused.chain3_order; the processing order
 * of regnet_sa_chain3_f32) -- as a three-bin counting sort in one launch.  count (n) int64 device (regnet_ball_query_f32's
 * second output), n <= 2^24.                                                                                                 */
int regnet_class_order_i64(const int64_t* count, int64_t n, int64_t* order, void* stream);

/* regnet_pair_order_i64: order (n) int64 = a processing order of the level-1 neighbourhoods for regnet_sa_chain3_f32's row
 * packing (fused.chain3_pair_order).  With ft = (count - 1) / 32 full point tiles and rem = (count - 1) % 32 + 1 remainder rows
 * per neighbourhood (count clamped to 1..64): neighbourhoods are paired greedily (ascending remainders; the smallest left
 * with the largest left when rem + rem' <= 32, else the largest stays without a partner; those go side by side two and two),
 * the pairs are sorted by their cost in point tiles (ft + ft' + 1 when they share a tile, ft + ft' + 2 otherwise; light first)
 * and pair p sits at slots 8 (p / 4) + p % 4 and + 4 (waves w and w + 4 of a chain workgroup); the n % 8 trailing slots take
 * the last pairs one after the other.  The result is a permutation of 0..n-1 and does not depend on timing.  One launch,
 * one workgroup.  count (n) int64 device, work (n) int32 device scratch, n <= 2^24.                                         */
int regnet_pair_order_i64(const int64_t* count, int64_t n, int64_t* order, int32_t* work, void* stream);

/* regnet_grasp_collision_counts_f32 / regnet_grasp_antipodal_stats_f32: the per-grasp point scans of the reference's grasp
 * evaluation, dataset_utils/eval_score/eval.py:4-24 -> eval_utils/evaluation_data_generator.py (EvalDataTest /
 * EvalDataValidate .finger_hand_view :188-236 / :420-483, .finger_hand_scene :485-537, ._antipodal_score :392-418;
 * constants: eval_score/configs/config.py), which loop over the grasps in Python.  test.py:147 applies the view-cloud
 * filter to every predicted grasp (utils.py:391-401); utils.py:270-295 scores validation grasps against the scene cloud.
 * points (and normals): N rows, element strides (pn, pc) / (nn, nc) for (point, coordinate); T (B,4,4) row-major
 * global->local matrices (:91-93).  With (x,y,z) = T[b] (p,1) and all comparisons strict, counts[b] (4 x int32) =
 *   { #(x_lo < x < x_hi), # behind the hand (.. and |y| < half_width, x < back_x, |z| < half_thickness),
 *     # inside a finger (.. |z| < half_thickness, half_space < |y| < half_width), # closing region (.. |y| < half_space) };
 * x_hi_per_grasp (B) overrides x_hi when not NULL (per-grasp depths, :428-430).  The caller applies the reference's
 * thresholds.  Antipodal statistics over the closing-region points: stats[b] = { y_max, y_min, sum |n_y| over
 * y > y_max - d, sum |n_y| over y < y_min + d } with d = min((y_max - y_min) / 3, neighbour_depth) and n_y the normal's
 * y component in the grasp frame; side_counts[b] = the two point counts (the reference's score is the product of the
 * two means).  fp32, individually rounded, no contraction; the sums are accumulated in fp64.                            */
int regnet_grasp_collision_counts_f32(const float* points, int64_t pn, int64_t pc, int64_t N, const float* T, int64_t B,
                                      float x_lo, float x_hi, const float* x_hi_per_grasp, float half_thickness,
                                      float half_width, float half_space, float back_x, int32_t* counts, void* stream);
int regnet_grasp_antipodal_stats_f32(const float* points, int64_t pn, int64_t pc, const float* normals, int64_t nn,
                                     int64_t nc, int64_t N, const float* T, int64_t B, float x_lo, float x_hi,
                                     const float* x_hi_per_grasp, float half_thickness, float half_width, float half_space,
                                     float back_x, float neighbour_depth, float* stats, int32_t* side_counts, void* stream);

/* Training twins (round 3).  regnet_gather_max_arg_f32: regnet_gather_max_f32 that also returns, per (row, channel), the
 * source row that gave the maximum (arg (R,F) int64; first maximum in group order; a negative row id counts from the end as
 * the reference's `all_feature.view(-1,F)[index]` does, gripper_region_network.py:382-390) -- the backward of the pooled
 * region feature then scatters R x F values.  regnet_rowsum_neg_f32: out[r] = -sum_k x[r*K + k] (K a power of two in
 * 4..256): the gradient of the per-centre term of a pre-multiplied first layer (dV = -sum over the K neighbours of dY). */
int regnet_gather_max_arg_f32(const float* feat, int64_t num_rows, int64_t F, const int64_t* rows, int64_t R, int64_t G,
                              float* out, int64_t* arg, void* stream);
/* regnet_scatter_max_grad_f32: the backward of regnet_gather_max_arg_f32 -- grad[arg[r][f]][f] += dy[r][f] for dy, arg (R, F)
 * (arg < 0: nothing), by float atomics.  Row `row` is scene b = row / scene_rows, point n = row % scene_rows and lands at
 * grad + b * batch_stride + n * row_stride + f * ch_stride: (scene_rows = total rows, row_stride F, ch_stride 1) for a
 * (rows, F) matrix, (scene_rows N, batch_stride F * N, row_stride 1, ch_stride N) for the channel-first (B, F, N) gradient
 * of the feature map itself.  grad is ADDED to (zero it, or hand in a gradient that is to receive this one).           */
int regnet_scatter_max_grad_f32(const float* dy, const int64_t* arg, int64_t R, int64_t F, int64_t scene_rows,
                                int64_t batch_stride, int64_t row_stride, int64_t ch_stride, float* grad, void* stream);
int regnet_rowsum_neg_f32(const float* x, int64_t rows, int64_t K, float* out, void* stream);

/* regnet_heads_chain_f32: a small tree of conv(1x1) + folded eval BatchNorm (+ ReLU) layers over FEW rows in one launch -- the
 * grasp heads of the region stage (pointnet2.py:174-188: 256 -> 1024 -> {256 -> 128 -> k_cls | 256 -> 128 -> k_reg};
 * pointnet2.py:240-253: 384 -> 1024 -> {128 -> k_cls | 128 -> k_reg}) on the B * 64 centres / the valid crops.  A workgroup
 * takes 16 rows through all layers; activations stay in LDS.  x (n, Kx) rows with stride ldx (multiple of 4, 16-byte
 * aligned); descr: `layers` (<= 8) records of 9 int64 [W, scale, shift (device addresses: W packed [>= ceil16(N)][Kpad] zero
 * padded, scale / shift [N]: y = relu?(scale * (W . x) + shift)), K, Kpad (multiple of 16), N, relu, src, dst]; buffers: 0 =
 * input, 1..3 = LDS scratch (a scratch buffer's width is its producer's N rounded up to 16 and must equal its consumers'
 * Kpad), dst 4 / 5 = out_a (n, lda) / out_b (n, ldb).  Layers run in order.  REGNET_ERR_UNSUPPORTED beyond 160 KiB of LDS. */
int regnet_heads_chain_f32(const float* x, int64_t ldx, int64_t Kx, int64_t n, const int64_t* descr, int64_t layers,
                           float* out_a, int64_t lda, float* out_b, int64_t ldb, void* stream);

/* regnet_heads_tree_f32: the same two trees for MANY rows (the 512 centres of 8 scenes, the 4000 of test.py:68) in one launch.
 * A workgroup takes 32 rows; the wide trunk activation (pointnet2.py:174 / :240: 1024 columns) is produced 256 columns at a
 * time and consumed at once by BOTH branches' first layers, whose weights the caller concatenates row-wise (N2 = 512 for
 * 1024 -> 256 | 256, 256 for 1024 -> 128 | 128); their outputs accumulate in registers, so no row count needs the trunk in
 * LDS and every weight fragment feeds two row blocks.  Same operand mapping and K order as regnet_heads_chain_f32: same bits.
 * descr: (2 + tails) records of 11 int64 [W, scale, shift (device addresses, packed as above), K, Kpad, N, relu, src,
 * src_off, dst, dst_off]; record 0 = trunk (K = Kx, Kpad = ceil16(Kx), N = Nt a multiple of 256), record 1 = the joined
 * first layers (K = Kpad = Nt, N = N2 in {256, 512}), then tails <= 4 in execution order with src 0 = the stage-2 rows / 1 =
 * the tail buffer read from column src_off (multiple of 4) on, dst 1 = the tail buffer at column dst_off, 4 / 5 = out_a (n,
 * lda) / out_b (n, ldb).  REGNET_ERR_UNSUPPORTED beyond 160 KiB of LDS.                                                  */
int regnet_heads_tree_f32(const float* x, int64_t ldx, int64_t Kx, int64_t n, const int64_t* descr, int64_t tails,
                          float* out_a, int64_t lda, float* out_b, int64_t ldb, void* stream);

/* The same heads in TRAINING mode, one layer per call (pointnet2.py:174-188, :240-253: nn.Conv1d(K, N, 1) with bias ->
 * nn.BatchNorm1d(N) on batch statistics -> [ReLU], on the R labelled centres / valid crops of the iteration): six launches
 * per layer forward and seven backward through torch, on a stream the host paces.
 * regnet_head_layer_train_supported: 2 <= R <= 1024, K a multiple of 64, N >= 1.
 * regnet_head_layer_train_fwd_f32: X (R, K) rows with stride ldx (multiple of 4; X and W 16-byte aligned), W (N, K), bias
 *   (N) or NULL -> xhat (R, N) the normalised pre-affine activation, Y (R, N) = [relu](gamma * xhat + beta), save_invstd (N);
 *   running_mean / running_var (both or neither) are updated in place with `momentum` (running_var from the unbiased
 *   variance, running_mean from mean(X . W^T) + bias), *num_batches_tracked (device int64, may be NULL) is incremented.
 * regnet_head_layer_train_bwd_f32: dY (R, N) with row stride lddy = the gradient of Y; Y is read for the ReLU mask only
 *   (may be NULL when relu == 0) -> dZ (R, N) the gradient of the convolution's output (workspace of the call), dW (N, K),
 *   dbias (N, may be NULL), dgamma (N), dbeta (N), and, when dX != NULL, dX (R, K) with row stride lddx = dZ . W, ADDED to
 *   its contents when accumulate_dx != 0 (the second branch of a fork).  Deterministic: fixed summation orders. */
int regnet_head_layer_train_supported(int64_t R, int64_t K, int64_t N);
int regnet_head_layer_train_fwd_f32(const float* X, int64_t ldx, const float* W, const float* bias, const float* gamma,
                                    const float* beta, float* running_mean, float* running_var, int64_t* num_batches_tracked,
                                    float momentum, float eps, int64_t R, int64_t K, int64_t N, int relu, float* xhat, float* Y,
                                    float* save_invstd, void* stream);
int regnet_head_layer_train_bwd_f32(const float* dY, int64_t lddy, const float* Y, const float* xhat, const float* gamma,
                                    const float* save_invstd, const float* X, int64_t ldx, const float* W, int64_t R, int64_t K,
                                    int64_t N, int relu, float* dZ, float* dW, float* dbias, float* dgamma, float* dbeta,
                                    float* dX, int64_t lddx, int accumulate_dx, void* stream);

/* Decodes of the two grasp heads WITHOUT labels (inference), one launch each instead of ~25 / ~12 small tensor ops.
 * regnet_stage2_decode_f32 (gripper_region_network.py:69-90, `ground is None`): cls (n,A), reg (n,A,C >= 7), centre rows
 * (n, centre_ld >= 3), tmpl (A,4) = the anchors' [r | theta] -> out (n,C): the arg-max anchor's regression turned into
 * [delta*radius + centre | (delta + r)/sqrt(|.|^2 + 1e-12) | pi*(delta + theta) | channels 7..], the latter through a
 * sigmoid when sigmoid_tail != 0 (pointnet2.py:187, for a head that hands over raw values).
 * regnet_refine_decode_f32 (gripper_region_network.py:201-215): grasp (n, grasp_ld >= C), cls (n,2), reg (n,C >= 8) ->
 * final_grasp (n,C) = grasp + deltas (the first three times radius), flags (2,n) uint8: [class 1 | class 1 and
 * final[:,7] > score_thre].                                                                                            */
int regnet_stage2_decode_f32(const float* cls, const float* reg, int64_t A, int64_t C, const float* centre,
                             int64_t centre_ld, const float* tmpl, float radius, int sigmoid_tail, int64_t n, float* out,
                             void* stream);
int regnet_refine_decode_f32(const float* grasp, int64_t grasp_ld, const float* cls, const float* reg, int64_t C,
                             float radius, float score_thre, int64_t n, float* final_grasp, uint8_t* flags, void* stream);

/* The two grasp losses of the training iteration with their gradients (csrc/losses.hip; gripper_region_network.py:46-184,
 * :186-309 with labels).  Every row-wise quantity in one launch, the class-balanced cross entropy in a second one after the
 * host's numpy draws; smooth-L1 is torch's default (beta 1), 1 - cos as compute_cos_sim / CosineEmbeddingLoss write it.
 * regnet_stage2_loss_rows_f32: cls (n,A), reg (n,A,10), centre rows (n, centre_ld), tmpl (A,4), label rows (n, label_ld >= 10),
 *   rows (m) int64 = the labelled centres (NULL: all n = m), weights4 = the four regression terms' weights (host pointer) ->
 *   compact per labelled centre: next_grasp (m,10) (arg-max decode), pick / g8 (m) int32 (arg-max class / label's anchor),
 *   a_gt (m,7), terms (m,12) = [4 regression terms | 4 monitoring terms | g8 == pick | 0 0 0]; dreg (n,A,10) rows `rows` =
 *   gradient of the weighted regression terms (other rows untouched: zero-fill first).
 * regnet_ce_rows_f32: loss[k] = CE(cls[rows[idx[k]]], target[idx[k]]), dcls[rows[idx[k]], :] = (softmax - onehot) * scale.
 * regnet_refine_loss_rows_f32: grasp rows (m, ld), cls (m,2), reg (m,10), label rows -> final_grasp (m,10), flags (3,m) uint8
 *   [class 1 | class 1 and score kept | label-positive], terms (m,20) = [4 regression terms of positive rows | 3 x 4
 *   monitoring terms | 4 confusion counts], dreg (m,10) = SL1' of the positive rows' residuals (unscaled).            */
/* regnet_label_match_f32: the training labels of the centres (dataset_utils/get_regiondataset.py:45-134, :136-199 with
 * use_theta): packed (B, Gmax, 19) = the scenes' ground-truth grasps padded to the longest record [16 row-major entries of the
 * 4x4 frame | score | antipodal score | centre score], gcount (B) their counts, centre rows at centre + b * centre_sb + c *
 * centre_sn (xyz first) -> out (B, Nc, 10) = [grasp centre | closing axis with x >= 0 | angle in (-pi, pi] | 3 scores] of the
 * grasp whose contact point is nearest (the reference's fp32 expansion compared as float64, first minimum), or the reference's
 * filler (-1, axis +1) when that squared distance exceeds max_sq; wide_row (B * Nc) = 1 where the row's antipodal score is not
 * -1 (the reference returns 8 channels when none is).  Replaces ~60 tensor launches. */
int regnet_label_match_f32(const float* packed, const int32_t* gcount, int64_t Gmax, const float* centre, int64_t centre_sb,
                           int64_t centre_sn, int64_t B, int64_t Nc, float depth, double max_sq, float* out,
                           int32_t* wide_row, void* stream);
int regnet_stage2_loss_rows_f32(const float* cls, const float* reg, int64_t A, int64_t C, const float* centre,
                                int64_t centre_ld, const float* tmpl, const float* label, int64_t label_ld, float radius,
                                const float* weights4, const int64_t* rows, int64_t m, float* next_grasp, int32_t* pick,
                                int32_t* g8, float* a_gt, float* terms, float* dreg, void* stream);
int regnet_ce_rows_f32(const float* cls, int64_t A, const int32_t* target, const int64_t* idx, const int64_t* rows,
                       int64_t nb, float scale, float* loss, float* dcls, void* stream);
int regnet_refine_loss_rows_f32(const float* grasp, int64_t grasp_ld, const float* cls, const float* reg, const float* label,
                                int64_t label_ld, int64_t C, float radius, float score_thre, int64_t m, float* final_grasp,
                                uint8_t* flags, float* terms, float* dreg, void* stream);

/* regnet_gripper_frame_f32: grasp (n, ld >= 7) rows [centre | closing axis | theta | ...] -> centre (n,3), rot (n,3,3) with rows
 * [approach; axis_y; minor_normal] -- the frame maths of get_gripper_region_transform (gripper_region_network.py:447-506) in
 * one launch.  regnet_crop_pick: the drawn candidate positions of a box crop resolved to group positions and scene indices
 * (index / index_inall (n,R) int64; -1 rows for grasps whose crop is invalid; :540-548). */
int regnet_gripper_frame_f32(const float* grasp, int64_t ld, int64_t n, float* centre, float* rot, void* stream);
int regnet_crop_pick(const int32_t* cand, int64_t G, const int64_t* pos, int64_t R, const uint8_t* valid,
                     const int64_t* group_index, int64_t gi_stride, int64_t n, int64_t* index, int64_t* index_inall,
                     void* stream);

/* regnet_resample_groups_f32: the gather half of get_regiondataset.py:331-352 (_get_group_pc).  cand (B,Nc,cap) int32: the
 * ascending member lists of regnet_radius_group_f32; pos (B,Nc,G) int64: positions into them drawn on the host with numpy's
 * RNG stream (-1 in every slot of a centre without candidates); pc (B,N,C) rows with element strides (pb, pn), channels
 * contiguous.  index[b,c,g] = cand[b,c,pos[b,c,g]] and points[b,c,g,:] = pc[b,index,:], or -1 / -1.0f where pos < 0 (the
 * reference fills empty groups with -1, :346-350).  Replaces seven tensor ops per pass.
 * A position >= cap or a candidate outside [0, N) (an upstream count / capacity mismatch; the torch.gather this replaces
 * raised on it) reads nothing, yields -1 and ORs 1 into *out_of_range (device int32, may be NULL).                       */
int regnet_resample_groups_f32(const float* pc, int64_t pb, int64_t pn, int64_t C, const int32_t* cand, int64_t cap,
                               const int64_t* pos, int64_t B, int64_t Nc, int64_t G, int64_t N, int32_t* out_of_range,
                               int64_t* index, float* points, void* stream);

/* regnet_estimate_normals_f32: surface normals of a scene cloud for validation records that carry no scene_normal --
 * dataset_utils/eval_score/eval_utils/torch_scene_point_cloud.py:17-19 -> eval_utils/pointcloud.py:27-43, i.e. open3d's
 * estimate_normals(KDTreeSearchParamHybrid(radius = NORMAL_RADIUS, max_nn = NORMAL_MAX_NN)), normalize_normals and
 * orient_normals_towards_camera_location (configs/config.py:16-17).  open3d is a dependency outside the reference tree
 * (absent from this image: parity unpinned, see oracle/collision_oracle.py); the algorithm restated is its published one:
 * neighbours of point i = the max_nn nearest points (itself included) with squared distance -- double,
 * ((dx*dx)+(dy*dy))+(dz*dz) -- strictly below float(radius*radius), ties ranked by index; fewer than 3 neighbours ->
 * (0,0,1); otherwise the eigenvector of the smallest eigenvalue of the neighbours' covariance (second moments / n -
 * mean products, double), a zero vector replaced by (0,0,1); normalised; negated when it points away from the camera
 * (normal . (camera - point) < 0).  xyz (N,3) contiguous float32, normals (N,3) float32, count (N) int32 = neighbours
 * used (may be NULL).  workspace: regnet_normals_workspace_bytes(N) bytes, 16-byte aligned.  max_nn <= 64.             */
int64_t regnet_normals_workspace_bytes(int64_t N);
int regnet_estimate_normals_f32(const float* xyz, int64_t N, double radius, int64_t max_nn, double cam_x, double cam_y,
                                double cam_z, float* normals, int32_t* count, void* workspace, void* stream);

/* regnet_bn_relu_train_fwd_f32 / _bwd_f32: TRAINING-mode BatchNorm (+ ReLU, + max over the K neighbours) of a shared-MLP
 * block -- nn/modules/conv.py:30-36, :70-76 (bn then relu after the bias-free 1x1 convolution) and the set-abstraction
 * reduction torch.max(new_feature, 3) of modules.py:245 -- as two HBM passes each way instead of torch's 13-18.
 * x (B, C, L) contiguous, 16-byte aligned; statistics per channel over (B, L), biased variance for the normalisation,
 * running_mean / running_var (may be NULL) updated with `momentum` and the unbiased variance, save_mean / save_invstd
 * (C) written for the backward.  pool_group == 0: y (B, C, L) = [relu](bn(x)).  pool_group = K (a power of two in
 * 4..256 dividing L, the K neighbours innermost): y (B, C, L/K) = max over each run of K, pool_index (B, C, L/K) int32 =
 * position of the selected element (smallest on ties).  workspace: regnet_bn_workspace_bytes(C) bytes.
 * Backward: dy shaped like y; dx (B, C, L), dgamma / dbeta (C) are overwritten; the ReLU mask is recomputed from x
 * (pooled: taken from y, which must then be the forward's output).                                                   */
int64_t regnet_bn_workspace_bytes(int64_t C);
int regnet_bn_relu_train_fwd_f32(const float* x, int64_t B, int64_t C, int64_t L, const float* gamma, const float* beta,
                                 float eps, float momentum, float* running_mean, float* running_var, int relu,
                                 int64_t pool_group, float* y, int32_t* pool_index, float* save_mean, float* save_invstd,
                                 void* workspace, void* stream);
int regnet_bn_relu_train_bwd_f32(const float* x, const float* y, const float* dy, const int32_t* pool_index, int64_t B,
                                 int64_t C, int64_t L, const float* gamma, const float* beta, const float* save_mean,
                                 const float* save_invstd, int relu, int64_t pool_group, float* dx, float* dgamma,
                                 float* dbeta, void* workspace, void* stream);

/* The statistics half of regnet_bn_relu_train_fwd_f32 alone, plus the normalisation as a per-channel affine
 * (scale = gamma * invstd, shift = beta - mean * scale), for the convolution that consumes the BatchNorm's output and applies
 * it to its own operand (regnet_conv1x1_fwd_bnrelu_stream_f32 / regnet_conv1x1_wgrad_bnrelu_f32 below): conv -> bn -> relu ->
 * conv of nn/modules/mlp.py:95-107 without writing the normalised activation.  The backward is regnet_bn_relu_train_bwd_f32
 * on the input gradient of that convolution.                                                                           */
int regnet_bn_train_stats_f32(const float* x, int64_t B, int64_t C, int64_t L, const float* gamma, const float* beta, float eps,
                              float momentum, float* running_mean, float* running_var, float* save_mean, float* save_invstd,
                              float* scale, float* shift, void* workspace, void* stream);
/* ..._from_sums: the same two entry points with the statistics PASS already done -- `workspace` holds, per channel, the sum and
 * the sum of squares of x over all B L elements (2 C doubles) as regnet_conv1x1_fwd_stats_stream_f32, the convolution that
 * produced x, accumulated them from its output tiles: x is not read for its statistics (regnet_bn_train_stats_from_sums_f32
 * does not take it at all).                                                                                            */
int regnet_bn_relu_train_fwd_from_sums_f32(const float* x, int64_t B, int64_t C, int64_t L, const float* gamma, const float* beta,
                                           float eps, float momentum, float* running_mean, float* running_var, int relu,
                                           int64_t pool_group, float* y, int32_t* pool_index, float* save_mean,
                                           float* save_invstd, void* workspace, void* stream);
int regnet_bn_train_stats_from_sums_f32(int64_t B, int64_t C, int64_t L, const float* gamma, const float* beta, float eps,
                                        float momentum, float* running_mean, float* running_var, float* save_mean,
                                        float* save_invstd, float* scale, float* shift, void* workspace, void* stream);

/* ---- set-abstraction layers 1+2 with layer 1 evaluated per SOURCE point ---------------------------
 * The first SharedMLP layer of a set-abstraction block (pn2_utils/modules.py:44-55: conv over
 * [xyz_j - xyz_c | feature_j]) is linear in the gathered row, so
 *   scale1 * W1 [f_j | x_j - x_c] + shift1 = U[j] - V[c],   U = scale1 * W1 [f | x]  (B*Nsrc rows),
 *                                                             V = scale1 * W1x x_c - shift1 (B*M rows),
 * both produced by regnet_mlp_layer_f32 (relu = 0).  This entry point gathers, applies the ReLU and
 * multiplies by layer 2:  A[p][k] = max(U[b*Nsrc + nbr[p]][k] - V[p / group][k], 0), k < C1 (C1 % 4 == 0);
 * C = epilogue(A . W^T) exactly as regnet_mlp_layer_f32 (pool_group 0 or 64).  Same values as the
 * gather-then-multiply form up to fp32 rounding of the re-associated sum.                          */
int regnet_sa_premul_layer_f32(const float* U, int64_t ldu, const float* V, int64_t ldv, int64_t C1,
                               const int64_t* nbr, int64_t B, int64_t Nsrc, int64_t M, int64_t group,
                               const float* W, int64_t Kpad, const float* scale, const float* shift,
                               float* C, int64_t ldc, int64_t N, int relu, int pool_group, void* stream);

/* regnet_interp_concat_f32: FeatureInterpolator.forward (modules.py:104-131) channels-last:
 * out[b*Nd+n] = [sum_k w_k * sparse[b, idx[b,n,k], 0:Cs] | dense[b,n,0:Cd] | 0...], w from squared
 * distances (inv = 1/max(d2,eps), w = inv/sum).  sparse (b,n,:) at sparse[b*sb + n*sn + c];
 * dense element (b,n,c) at dense[b*db + n*dn + c*dc]; out row stride ldo >= Cout >= Cs+Cd.        */
int regnet_interp_concat_f32(const float* sparse, int64_t sb, int64_t sn, int64_t Cs,
                             const int64_t* idx, const float* dist2, float eps, const float* dense,
                             int64_t db, int64_t dn, int64_t dc, int64_t Cd, int64_t B, int64_t Nd,
                             float* out, int64_t ldo, int64_t Cout, void* stream);

/* ---- feature propagation with the first SharedMLP layer applied BEFORE the interpolation -------------
 * The layer is linear in [sum_k w_k sparse[idx_k] | dense] (pn2_utils/modules.py:117-131), hence
 *   out[p][n] = relu(scale[n] * (sum_k w_k Ys[b, idx_k[p]][n] + Yd[p][n]) + shift[n]),
 * Ys (B,Ns,C) = Ws . sparse per SPARSE point (strides sb,sn; channel stride 1), Yd (B*Nd, ldd) = Wd . dense
 * per dense point or NULL, both from regnet_mlp_layer_f32 with scale 1 / shift 0 / relu 0; w_k as in
 * regnet_interp_concat_f32 (from squared distances).  A narrow skip input (Cd_small <= 4 channels, e.g.
 * rgb; element (b,c,n) at dense_small[b*db + c*dc + n*dn]) is multiplied in place with its weight columns
 * Wd4 (C x 4, zero padded) instead of going through Yd; pass NULL when unused.
 * C % 4 == 0, C/4 must divide 256.  out (B*Nd, ldo).                                                   */
int regnet_interp_affine_f32(const float* ys, int64_t sb, int64_t sn, const int64_t* idx,
                             const float* dist2, float eps, const float* yd, int64_t ldd,
                             const float* dense_small, int64_t db, int64_t dn, int64_t dc,
                             int64_t Cd_small, const float* Wd4, const float* scale, const float* shift,
                             int relu, int64_t B, int64_t Nd, int64_t C, float* out, int64_t ldo,
                             void* stream);

/* regnet_score_head_f32: score = sigmoid(bn_score(conv_score(x))) (utils/pointnet2.py:117-119),
 * x (P,C) channels-last, w (C), bn folded to (bn_scale, bn_shift).                                */
int regnet_score_head_f32(const float* x, int64_t ldx, int64_t C, const float* w, float bias,
                          float bn_scale, float bn_shift, float* score, int64_t P, void* stream);

/* regnet_sa_premul_chain_f32: layers 2 and 3 + the max over the 64 neighbours of the level-2 set-abstraction block of
 * PointNet2Seg (utils/pointnet2.py:40-42: sa_channels[1] = (256, 256, 512); pn2_utils/modules.py:39-56, :244-245) in one
 * kernel, on pre-multiplied layer-1 rows as regnet_sa_premul_layer_f32 takes them:
 *     x0[p] = relu(U[b * Nsrc + nbr[p]] - V[p / 64])  ->  256 -> 256 -> 512 (folded BN affine, ReLU; ReLU of the last
 *     layer if relu3)  ->  out[p / 64] = max over the neighbourhood.
 * U (B*Nsrc, ldu >= 256), V (B*M, ldv >= 256), nbr (B, M, 64) int64, out (B*M, ldo >= 512).  Activations stay in
 * registers (csrc/rowchain.hip); the (B*M*64 x 256) layer-2 activation of the two-launch path is never written.
 * `stream_w`: regnet_sa_premul_chain_stream_floats() floats = 24 stages [32 output channels][256 k] -- the 8 row
 * blocks of W2, then the 16 of W3 -- chunk-swizzled like regnet_fp_head_chain_f32's; `affine` = [scale2 | shift2 |
 * scale3 | shift3] (1536 floats); `ticket`: one zeroed int32 (work-queue head).  Same values as
 * regnet_sa_premul_layer_f32 + regnet_mlp_layer_f32(pool) up to fp32 summation order.                              */
int64_t regnet_sa_premul_chain_stream_floats(void);
int regnet_sa_premul_chain_f32(const float* U, int64_t ldu, const float* V, int64_t ldv, const int64_t* nbr, int64_t B,
                               int64_t Nsrc, int64_t M, const float* stream_w, int64_t n_stages, const float* affine,
                               int64_t affine_floats, int relu3, float* out, int64_t ldo, int32_t* ticket,
                               void* stream);

/* regnet_sa3_premul_chain_f32: the same for the level-3 block (utils/pointnet2.py:40-42: 515 -> 512 -> 512 -> 1024 over
 * 256 x 64 rows per scene): U (B*Nsrc, >=512), V (B*M, >=512) pre-multiplied layer-1 rows as for
 * regnet_sa_premul_layer_f32; layer 2 (512 -> 512) runs as two K-halves so that its 512-wide activation stays in
 * registers, layer 3 (512 -> 1024) point-major with the max over the 64 neighbours; out (B*M, 1024).
 * `stream_w`: regnet_sa3_premul_chain_stream_floats() floats = 96 stages [32 output channels][256 k]: W2 as
 * (K-half, 16 row blocks), then W3 as (32 row blocks, K-half); `affine` = [scale2 | shift2 | scale3 | shift3]
 * (3072 floats).  Same values as regnet_sa_premul_layer_f32 + regnet_mlp_layer_f32(pool) up to fp32 summation order. */
int64_t regnet_sa3_premul_chain_stream_floats(void);
int regnet_sa3_premul_chain_f32(const float* U, int64_t ldu, const float* V, int64_t ldv, const int64_t* nbr, int64_t B,
                                int64_t Nsrc, int64_t M, const float* stream_w, int64_t n_stages, const float* affine,
                                int64_t affine_floats, int relu3, float* out, int64_t ldo, int32_t* ticket,
                                void* stream);

/* regnet_fp_head_chain_f32: the tail of the last feature-propagation block and the whole segmentation head of
 * PointNet2Seg as ONE kernel (utils/pointnet2.py:64-84 with fp_channels[2] = (256, 256, 256), :116-119 with
 * seg_channels = (512, 256, 256, 128); pn2_utils/modules.py:500-509):
 *     X (P, 256: the block's first layer, e.g. from regnet_interp_affine_f32) -> 256 -> 256 = F (P, 256), the point
 *     feature ScoreNetwork returns -> 512 -> 256 -> 256 -> 128 -> conv_score + bn_score + sigmoid = score (P).
 * Every layer is a bias-free 1x1 convolution + eval BatchNorm (folded to scale/shift) + ReLU.  A wave keeps the
 * activations of 16 points in registers from X to the score (csrc/rowchain.hip); only X is read and only F / score
 * are written -- the layer-wise path moves 15x the bytes.  Same values as six regnet_mlp_layer_f32 calls +
 * regnet_score_head_f32 up to fp32 summation order.
 * `stream_w`: regnet_fp_head_chain_stream_floats() floats = 60 stages of 32 KiB in consumption order -- per layer
 * pair (A: 256 -> M, B: M -> N) and per 128-channel group g of M: four A-stages (rows 128 g + 32 u .. + 32 of W_A, all
 * 256 columns) then N/64 B-stages (rows 64 v .. + 64 of W_B, columns 128 g .. + 128); inside a stage the 16-byte
 * chunk c of row r is stored at chunk position c ^ (r & 15) (low 4 bits) of its row (bank-conflict-free fragment
 * reads).  `affine`: per layer [scale(N) | shift(N)], layers in order: 3328 floats.  Rows and buffers 16-byte aligned.
 * `ticket`: one int32 in device memory, ZERO when the kernel starts (the caller clears it on the same stream): the
 * work queue through which the resident workgroups draw their 128-row blocks.                                          */
int64_t regnet_fp_head_chain_stream_floats(void);
/* A launch hands out the 128-row blocks [block_first, block_first + block_count) of the regnet_fp_head_chain_blocks(P) the
 * rows make (block_count < 0: all of them).  Two launches over disjoint ranges, each with its OWN zeroed ticket word, may
 * run on different streams: the caller can put the last, partial round of blocks (P = 204 800 rows: 1600 blocks = 6 x 256 +
 * 64) beside whatever its main stream runs next instead of leaving 3/4 of the chip idle for a whole pass.            */
int64_t regnet_fp_head_chain_blocks(int64_t P);
/* regnet_fp_head_chain_interp_f32: the same chain with the block's FIRST layer in its prologue -- 3-NN interpolation of
 * the pre-multiplied sparse rows + the narrow skip input + folded BN + ReLU, i.e. regnet_interp_affine_f32's arithmetic
 * (pn2_utils/modules.py:104-131, :500-509) -- so that the (P x 256) first-layer activation is never written:
 * Ys (B, Ns, 256) with element strides ys_sb / ys_sn; idx / dist2 (B*Nd, 3); dense_small (B, Cd <= 4, Nd) with element
 * strides db / dn / dc or NULL; tables = Wd4 (256 x 4) | scale1 (256) | shift1 (256); everything else as above.        */
int regnet_fp_head_chain_interp_f32(const float* Ys, int64_t ys_sb, int64_t ys_sn, const int64_t* idx,
                                    const float* dist2, float eps, const float* dense_small, int64_t db, int64_t dn,
                                    int64_t dc, int64_t Cd_small, const float* tables, int64_t B, int64_t Nd,
                                    const float* stream_w, int64_t n_stages, const float* affine, int64_t affine_floats,
                                    const float* wscore, float score_bias, float score_bn_scale, float score_bn_shift,
                                    float* F, int64_t ldf, float* score, int32_t* ticket, int64_t block_first,
                                    int64_t block_count, void* stream);
int regnet_fp_head_chain_f32(const float* X, int64_t ldx, const float* stream_w, int64_t n_stages,
                             const float* affine, int64_t affine_floats, const float* wscore, float score_bias,
                             float score_bn_scale, float score_bn_shift, float* F, int64_t ldf, float* score,
                             int64_t P, int32_t* ticket, int64_t block_first, int64_t block_count, void* stream);

/* ---- training: the 1x1 convolutions of the shared-MLP blocks on the matrix cores (csrc/tgemm.hip) ------------------
 * nn.Conv1d / nn.Conv2d(kernel_size = 1, bias = False) of pn2_utils/nn/modules/conv.py:20-36, :60-76 under autograd
 * (train.py:376-384), in the tensors' own channel-first layout: X (B, Ci, L), W (Co, Ci), Y (B, Co, L), all contiguous.
 *   fwd    Y[b]  = W . X[b]            dgrad  dX[b] = W^T . dY[b]            wgrad  dW = sum_b dY[b] . X[b]^T
 * regnet_conv1x1_train_supported(Co, Ci, L) != 0: this build runs the shape (channel counts multiples of 16 and >= 32,
 * L a multiple of 4 and >= 64; wgrad additionally L % 16 == 0); otherwise the entry points return REGNET_ERR_SHAPE and
 * the caller keeps its library GEMM.  The weight gradient is split over the point axis into
 * regnet_conv1x1_wgrad_slices() slices per scene whose partial sums (workspace of
 * regnet_conv1x1_wgrad_workspace_bytes() bytes, 16-byte aligned; may be NULL when that is 0) are added in slice
 * order by a second kernel: deterministic.  Same values as the library path up to fp32 summation order.          */
int regnet_conv1x1_train_supported(int64_t Co, int64_t Ci, int64_t L);
int regnet_conv1x1_fwd_f32(const float* W, const float* X, float* Y, int64_t B, int64_t Co, int64_t Ci, int64_t L,
                           void* stream);
int regnet_conv1x1_dgrad_f32(const float* W, const float* dY, float* dX, int64_t B, int64_t Co, int64_t Ci, int64_t L,
                             void* stream);
/* ..._stream: the same two contractions by the persistent kernel (two workgroups per CU draw output tiles from `ticket`,
 * an int32 zeroed by the caller, and keep one LDS ring running across tiles); bit-identical results.                  */
int regnet_conv1x1_fwd_stream_f32(const float* W, const float* X, float* Y, int64_t B, int64_t Co, int64_t Ci, int64_t L,
                                  int32_t* ticket, void* stream);
int regnet_conv1x1_dgrad_stream_f32(const float* W, const float* dY, float* dX, int64_t B, int64_t Co, int64_t Ci, int64_t L,
                                    int32_t* ticket, void* stream);
/* regnet_conv1x1_fwd_smallci_f32: the same forward for 1 <= Ci <= 8 input channels (the level-1 block's first layer on its
 * grouped rows, 6 -> 128): a store stream -- a thread holds four points of every input channel and writes a float4 per output
 * channel.  L % 4 == 0, X and Y 16-byte aligned, any Co.                                                                */
int regnet_conv1x1_fwd_smallci_f32(const float* W, const float* X, float* Y, int64_t B, int64_t Co, int64_t Ci, int64_t L,
                                   void* stream);
/* ..._stats: the same, also leaving sums (2 Co doubles, as regnet_conv1x1_fwd_stats_stream_f32 below) for the BatchNorm that follows.
 * Y = W X is linear in <= 8 inputs: the sums follow from the first and second moments of X (Ci + Ci (Ci + 1) / 2 numbers, fp64
 * above 256 points), Y is not read.  workspace: regnet_conv1x1_smallci_stats_workspace_bytes(B, Ci, L) bytes, 8-byte aligned. */
int64_t regnet_conv1x1_smallci_stats_workspace_bytes(int64_t B, int64_t Ci, int64_t L);
int regnet_conv1x1_fwd_smallci_stats_f32(const float* W, const float* X, float* Y, int64_t B, int64_t Co, int64_t Ci, int64_t L,
                                         void* workspace, void* sums, void* stream);
/* ... and their weight gradient: dW = sum over part's first axis, part (regnet_conv1x1_wgrad_smallci_partials(B, Co, L), Co, Ci)
 * written by the call (one partial matrix per scene and slice of the point axis; the caller's sum fixes the order).     */
int64_t regnet_conv1x1_wgrad_smallci_partials(int64_t B, int64_t Co, int64_t L);
int regnet_conv1x1_wgrad_smallci_f32(const float* dY, const float* X, float* part, int64_t B, int64_t Co, int64_t Ci, int64_t L,
                                     void* stream);
/* regnet_conv1x1_smallco_f32: the mirror case, 1 <= Co <= 4 output channels (the segmentation head's score convolution, 128 -> 1
 * with bias): dir 0: out (B, Co, L) = W (Co, Ci) . in (B, Ci, L) + bias (Co, may be NULL); dir 1: out (B, Ci, L) = W^T . in
 * (B, Co, L), the input gradient (bias ignored).  L % 4 == 0, in / out 16-byte aligned.  The weight gradient is
 * regnet_conv1x1_wgrad_smallci_f32 with the operands' roles swapped.                                                   */
int regnet_conv1x1_smallco_f32(int dir, const float* W, const float* bias, const float* in, float* out, int64_t B, int64_t Co,
                               int64_t Ci, int64_t L, void* stream);
/* regnet_conv1x1_stream_reserve_slots: the persistent kernels above hold every CU's register file for a whole launch (two
 * workgroups per CU); `slots` of those 2 x CUs workgroup slots stay empty from now on (at most half of them; negative: query
 * only), so that small kernels of ANOTHER stream -- the region stage beside the segmentation head's backward -- find CUs to
 * start on instead of advancing one launch per persistent launch.  Process-wide; returns the previous value.            */
int regnet_conv1x1_stream_reserve_slots(int slots);
/* EXPERIMENT, not on any default path (conv1x1_train.SPLIT_PRODUCTS): the same forward / input gradient with fp32-faithful
 * products on the bf16 matrix pipe -- every operand as the exact sum of three bf16 pieces, six of the nine piece products (the
 * dropped ones are <= 2^-24 relative), fp32 accumulation (csrc/tsplit.hip).  transposed == 0: Y (B, Co, L) = W (Co, Ci) .
 * X (B, Ci, L), optionally on [relu](bscale[i] X[., i, .] + bshift[i]) (NULL: none; Ci <= 1024); transposed == 1: dX (B, Ci, L) =
 * W^T . dY (B, Co, L).  Co, Ci multiples of 16.  workspace: regnet_conv1x1_split_workspace_bytes(Co, Ci, transposed) bytes,
 * 16-byte aligned (the weight's three bf16 planes, rebuilt by every call: the weights move every iteration).             */
/* ... and regnet_sa_chain3_f32 (the level-1 set-abstraction block in one kernel) the same way: csrc/sa_split.hip, fused.SPLIT_PRODUCTS,
 * off.  W2 (128 x 128, row stride ldw2) and W3 (C3 x 128, ldw3) are the packed fp32 weights; `planes`
 * (regnet_sa_chain3_split_plane_bytes(C3) bytes, 16-byte aligned) receives their bf16 pieces when build_planes != 0 and is read as it
 * is otherwise (the caller caches it per weight version).  ticket: a zeroed int32 (work-queue head of the persistent workgroups).
 * group == 64, Cf + 3 <= 8, C3 % 64 == 0.                                                                                  */
int64_t regnet_sa_chain3_split_plane_bytes(int64_t C3);
int regnet_sa_chain3_split_f32(const float* feat, int64_t fb, int64_t fn, int64_t fc, int64_t Cf, const float* xyz, int64_t xb,
                               int64_t xc, int64_t xn, const int64_t* nbr, const int64_t* ctr, const int64_t* count,
                               const int64_t* order, int64_t B, int64_t M, int64_t group,
                               const float* W1, const float* scale1, const float* shift1, const float* W2, int64_t ldw2,
                               const float* scale2, const float* shift2, const float* W3, int64_t ldw3, const float* scale3,
                               const float* shift3, int64_t C3, int relu3, void* planes, int build_planes, float* out, int64_t ldo,
                               int32_t* ticket, void* stream);
int regnet_conv1x1_split_supported(int64_t Co, int64_t Ci, int64_t L);
int64_t regnet_conv1x1_split_workspace_bytes(int64_t Co, int64_t Ci, int64_t transposed);
int regnet_conv1x1_split_f32(int transposed, const float* W, const float* in, float* out, int64_t B, int64_t Co, int64_t Ci,
                             int64_t L, const float* bscale, const float* bshift, int brelu, void* workspace, void* stream);
/* ..._bnrelu: the convolution's input is [relu](scale[i] * X[., i, .] + shift[i]) -- a training BatchNorm (+ ReLU) given as
 * its per-channel affine (regnet_bn_train_stats_f32) -- applied to the operand fragments inside the contraction; X itself
 * is the BatchNorm's INPUT.  regnet_conv1x1_bnrelu_supported: train_supported, Ci <= 512 (the affine table lives in LDS),
 * L % 16 == 0.                                                                                                         */
int regnet_conv1x1_bnrelu_supported(int64_t Co, int64_t Ci, int64_t L);
int regnet_conv1x1_fwd_bnrelu_stream_f32(const float* W, const float* X, float* Y, int64_t B, int64_t Co, int64_t Ci, int64_t L,
                                         const float* scale, const float* shift, int relu, int32_t* ticket, void* stream);
int regnet_conv1x1_wgrad_bnrelu_f32(const float* dY, const float* X, float* dW, int64_t B, int64_t Co, int64_t Ci, int64_t L,
                                    const float* scale, const float* shift, int relu, void* workspace, void* stream);
/* The forward (plain: scale == NULL; or ..._bnrelu) that also leaves the statistics of the BatchNorm FOLLOWING the convolution:
 * sums (2 Co doubles, 8-byte aligned; zeroed and filled by the call) = per output channel the sum and the sum of squares of Y
 * over all B L points, taken from the output tiles while they are in registers -- nn/modules/conv.py:30-36's bn(conv(x)) without
 * a statistics pass over Y.  Continue with regnet_bn_train_stats_from_sums_f32 / regnet_bn_relu_train_fwd_from_sums_f32.
 * regnet_conv1x1_fwd_stats_supported: train_supported, Co <= 256 (the fp64 table lives in LDS beside the operand ring);
 * affine: Ci <= 256, L % 16 == 0.                                                                                       */
int regnet_conv1x1_fwd_stats_supported(int64_t Co, int64_t Ci, int64_t L, int affine);
int regnet_conv1x1_fwd_stats_stream_f32(const float* W, const float* X, float* Y, int64_t B, int64_t Co, int64_t Ci, int64_t L,
                                        const float* scale, const float* shift, int relu, int32_t* ticket, void* sums,
                                        void* stream);
int64_t regnet_conv1x1_wgrad_slices(int64_t B, int64_t Co, int64_t Ci, int64_t L);
int64_t regnet_conv1x1_wgrad_workspace_bytes(int64_t B, int64_t Co, int64_t Ci, int64_t L);
int regnet_conv1x1_wgrad_f32(const float* dY, const float* X, float* dW, int64_t B, int64_t Co, int64_t Ci, int64_t L,
                             void* workspace, void* stream);

/* ---- host-side numpy-compatible random draws of the region stage (no GPU involved) ------------
 * Replaces the per-centre / per-grasp np.random.choice calls of the reference's Python loops
 * (dataset_utils/get_regiondataset.py:331-337, multi_model/gripper_region_network.py:532-544) while
 * consuming numpy's MT19937 stream identically.  mt_key[624] / mt_pos are np.random.get_state()[1:3]
 * (updated in place; the caller hands them back with np.random.set_state).  counts (rows) int32;
 * out (rows,size) int64 positions; valid (rows) u8 or NULL.  mode 0 = radius groups (n>=size: no
 * replacement, 0<n<size: replacement, n==0: -1), mode 1 = gripper crops (n>size / 5<n<=size / else
 * invalid).                                                                                       */
int regnet_np_choice_rows(uint32_t* mt_key, int32_t* mt_pos, const int32_t* counts, int64_t rows,
                          int64_t size, int mode, int64_t* out, uint8_t* valid);

/* ---- the same draws ON THE DEVICE (round 3): numpy's generator state lives in device memory ------
 * d_mt_key[624] (raw MT19937 words) / d_mt_pos[1] are np.random.get_state()[1:3] in device memory, updated in
 * place by kernels on `stream`; d_counts (rows) int32 device; d_out (rows,size) int64 device; d_valid (rows) u8 device
 * or NULL; semantics, row order and stream consumption exactly as regnet_np_choice_rows.  max_count bounds every
 * count (it sizes the workspace: regnet_np_choice_rows_dev_workspace_ints(rows, max_count) int32 words; the last
 * word is a status flag the caller may read back after the stream has drained: non-zero = a count exceeded
 * max_count and the results are invalid).  No host synchronisation.  Replaces the same reference loops
 * (dataset_utils/get_regiondataset.py:331-337, multi_model/gripper_region_network.py:532-544).            */
int64_t regnet_np_choice_rows_dev_workspace_ints(int64_t rows, int64_t max_count);
int regnet_np_choice_rows_dev(uint32_t* d_mt_key, int32_t* d_mt_pos, const int32_t* d_counts, int64_t rows,
                              int64_t size, int64_t max_count, int mode, int64_t* d_out, uint8_t* d_valid,
                              int32_t* d_workspace, void* stream);

/* regnet_np_rand_doubles_dev: np.random.rand(count) from the device-resident generator (two words per double,
 * randomkit's rk_double), d_out (count) float64 device.  Used by the device-side dataset item (scoredataset.py:52-58). */
int regnet_np_rand_doubles_dev(uint32_t* d_mt_key, int32_t* d_mt_pos, int64_t count, double* d_out, void* stream);

/* regnet_dataset_resample_f32: the gather + colour jitter + tanh of ScoreDataset.__getitem__
 * (dataset_utils/scoredataset.py:60-81) for one record on the device: cloud / color (M,3), score / label (M) float32
 * contiguous; pick (N) int64 rows drawn with numpy's stream; rand6 = the six np.random.rand() values of _noise_color
 * (:52-58: table gains, then the object draws r -> gain 1 - r / 5), float64 device.  Outputs pc (N,6) = [xyz | rgb *
 * gain], tanh(score) (N), label (N).  A pick outside [0, M) ORs 1 into *out_of_range (may be NULL).                 */
int regnet_dataset_resample_f32(const float* cloud, const float* color, const float* score, const float* label, int64_t M,
                                const int64_t* pick, int64_t N, const double* rand6, float* pc, float* score_out,
                                float* label_out, int32_t* out_of_range, void* stream);

/* ---- single-frame ingest (csrc/ingest.hip): the front end of the reference's test.py:101-129 on the device ----------
 * regnet_ingest_crop_f32 / regnet_ingest_crop_f64: rigid transform into the table frame (test.py:104) + workspace crop
 * (:114-118) of one raw camera frame as an order-preserving compaction.
 *   xyz, rgb   (M,3) contiguous DEVICE arrays, float32 (_f32) or float64 (_f64); float32 input is widened exactly.
 *   transform  HOST pointer, 16 doubles, row-major 4x4 (rows 0..2 are used: the reference's transform is rigid).
 *   bounds     HOST pointer, 5 doubles {x_hi, x_lo, z_hi, y_hi, y_lo}: a point is kept when x < x_hi, x > x_lo, z < z_hi,
 *              y < y_hi and y > y_lo, all strict, in the order of :114-118 (+-infinity switches a test off).
 *   drop_nonfinite != 0 drops rows with a NaN / infinite INPUT coordinate before the tests.  An explicit guard only: such a
 *              coordinate reaches x as NaN (also through 0 * inf) or as an infinity, and both fail a strict two-sided test.
 * Arithmetic (the translation unit is built with -ffp-contract=off): every coordinate is
 * ((T[r][0] x + T[r][1] y) + T[r][2] z) + T[r][3] in float64, each product and sum individually rounded; the tests are made
 * on those float64 values (the reference compares the float64 array).  Kept rows are written IN INPUT ORDER --
 * np.random.choice (:122-127) indexes this list:
 *   kept_xyz64 (M,3) float64, kept_xyz32 (M,3) float32 = kept_xyz64 rounded to nearest (torch.Tensor(pc), :129),
 *   kept_rgb (M,3) float64, kept_src (M) int32 source rows or NULL; rows from *count on are left untouched.
 *   count      (1) int32 DEVICE: the number of kept rows.  No host read, no synchronisation.
 *   workspace  regnet_ingest_crop_workspace_bytes(M) bytes, 8-byte aligned (per-wave ballots + per-workgroup counts).
 * Three launches (flags + counts, a one-workgroup exclusive scan, placement); no workgroup waits for another.
 * M == 0: *count = 0, nothing else touched (only `count`, `transform`, `bounds` must be non-NULL).  Nothing kept:
 * *count = 0.  Errors: M < 0 -> REGNET_ERR_SHAPE; M > 2^21 -> REGNET_ERR_UNSUPPORTED (the workspace size is then -1);
 * a NULL pointer for a required array -> REGNET_ERR_NULL.                                                              */
int64_t regnet_ingest_crop_workspace_bytes(int64_t M);
int regnet_ingest_crop_f32(const float* xyz, const float* rgb, int64_t M, const double* transform, const double* bounds,
                           int drop_nonfinite, double* kept_xyz64, float* kept_xyz32, double* kept_rgb, int32_t* kept_src,
                           int32_t* count, void* workspace, void* stream);
int regnet_ingest_crop_f64(const double* xyz, const double* rgb, int64_t M, const double* transform, const double* bounds,
                           int drop_nonfinite, double* kept_xyz64, float* kept_xyz32, double* kept_rgb, int32_t* kept_src,
                           int32_t* count, void* workspace, void* stream);
/* regnet_ingest_resample_f32: utils.noise_color (utils.py:426-431) + pc[select_point_index] + torch.Tensor(pc)
 * (test.py:120-129) as one gather: xyz (rows,3) float32, rgb (rows,3) float64 (rgb_is_f64 != 0: the real_data branch,
 * float64 product rounded to float32) or float32 (the record branch: numpy >= 2 multiplies the float32 column by the
 * float64 gain in double and rounds back to float32 -- the same value), pick (N) int64 drawn with numpy's stream, rand3 =
 * the three np.random.rand() values drawn BEFORE the choice (gain 1 - r / 5), float64; all device memory.  count (1) int32
 * device or NULL: the number of valid rows (at most `rows`; NULL = rows).  pc (N,6) float32 = [xyz | rgb * gain].  A pick
 * outside [0, count) -- the -1 rows an empty list draws, where np.random.choice raises -- writes a row of zeros and ORs 1
 * into *out_of_range (may be NULL); nothing is read out of bounds.  Errors: rows < 0 or N < 0 -> REGNET_ERR_SHAPE.     */
int regnet_ingest_resample_f32(const float* xyz, const void* rgb, int rgb_is_f64, const int32_t* count, int64_t rows,
                               const int64_t* pick, int64_t N, const double* rand3, float* pc, int32_t* out_of_range,
                               void* stream);
/* regnet_lzf_decompress: HOST code, the LZF codec of PCD `DATA binary_compressed` bodies (what open3d.io.read_point_cloud
 * does for test.py:102).  -> the number of bytes written to out (at most out_cap), or REGNET_ERR_SHAPE for a truncated /
 * corrupt stream or one that does not fit, REGNET_ERR_NULL for a NULL buffer of non-zero length.                          */
int64_t regnet_lzf_decompress(const uint8_t* in, int64_t in_len, uint8_t* out, int64_t out_cap);

/* ---- pose non-maximum suppression + top-K (csrc/nms.hip): the K best DISTINCT grasps of one set, on the device -------------
 * regnet_grasp_nms_f32: center (n,3) and frame (n,3,3) float32 contiguous -- eval_collision.grasp_frames' output, the frame's
 * COLUMNS being approach a, axis_y b and minor normal m --, order (n) int64 = the input row of every rank, best first (the
 * caller ranks: descending score, NaN as -inf, equal scores by lower row; entries outside [0, n) are never the same grasp as
 * anything).  Two grasps are the same grasp when they are close AND aligned, in individually rounded fp32 operations in the
 * written order (the translation unit is built with -ffp-contract=off):
 *   close    d2 = ((dx dx) + (dy dy)) + (dz dz) <= T2                      T2 = float32(t) * float32(t), inclusive
 *   aligned  tr = (da + db) + dm >= C, da = ((ax ax') + (ay ay')) + (az az') and likewise db, dm;
 *            C = 1 + 2 cos(theta) evaluated in float64 and rounded once to float32
 *            symmetric != 0: tr2 = (da - db) - dm, max(tr, tr2) >= C (a NaN in either fails it, as np.maximum): the gripper
 *            turned 180 degrees about its approach axis is the same grasp.
 * The ranks are walked in order; a rank is kept unless an already kept one is the same grasp; the walk stops once top_k are
 * kept (top_k <= 0: no limit).
 *   keep      (n) int64: the input rows of the kept grasps in rank order, then -1 up to n.
 *   count     (1) int32 DEVICE: how many were kept.  No host read, no synchronisation, no allocation: capturable.
 *   workspace regnet_grasp_nms_workspace_bytes(n) = nb (nb + 1) / 2 * 64 * 8 bytes with nb = ceil(n / 64), 8-byte aligned:
 *             one 64-bit word per (rank, later-or-own block of 64 ranks), the upper triangle of the pair mask; -1 for an
 *             unsupported n.  The callee writes all of it before reading.
 * Two launches (64 x 64 pair-mask tiles; a one-workgroup greedy scan that leaves early at top_k); no workgroup waits for
 * another.  n == 0: success, no pointer touched.  Errors: n < 0 -> REGNET_ERR_SHAPE; n > 32768 -> REGNET_ERR_UNSUPPORTED
 * (the workspace is 64.1 MiB there); a NULL pointer with n > 0 -> REGNET_ERR_NULL.  Validation precedes any launch.      */
int64_t regnet_grasp_nms_workspace_bytes(int64_t n);
int regnet_grasp_nms_f32(const float* center, const float* frame, const int64_t* order, int64_t n, float T2, float C,
                         int symmetric, int64_t top_k, int64_t* keep, int32_t* count, void* workspace, void* stream);

/* ---- table plane (csrc/plane.hip): the dominant support plane of one camera frame, on the device ---------------------------
 * regnet_plane_estimate_f32 / _f64: xyz (M,3) contiguous, float32 or float64 (a float64 value is rounded once to float32, to
 * nearest; everything below is on the float32 values).  A row with a non-finite float32 coordinate takes no part.  Canonical
 * fp32 arithmetic: individually rounded binary32 operations in the written order (-ffp-contract=off); dot(a, b) stands for
 * ((ax bx) + (ay by)) + (az bz).
 *   hypotheses  H of them, a multiple of 64, at most 4096.  Hypothesis h draws three rows: slot k = 0, 1, 2, attempt r = 0..7,
 *               z = splitmix64(seed * 2^32 + (3 h + k) * 8 + r) in uint64 arithmetic (x += 0x9E3779B97F4A7C15;
 *               x = (x ^ x >> 30) * 0xBF58476D1CE4E5B9; x = (x ^ x >> 27) * 0x94D049BB133111EB; z = x ^ x >> 31),
 *               row = ((z >> 32) * M) >> 32; the first attempt that hits a finite row fills the slot.  With an unfilled slot
 *               the hypothesis is invalid and its table row is zero.  Else a = p1 - p0, b = p2 - p0,
 *               n = ((ay bz) - (az by), (az bx) - (ax bz), (ax by) - (ay bx)), nn = dot(n, n); valid when 1e-12f < nn < inf.
 *   range gate  g = dot(p0, n): eligible when (lo lo) nn <= g g <= (hi hi) nn (float32 products; lo = 0, hi = inf: no gate).
 *   tilt gate   up_hint (3) float32 HOST memory or NULL (no gate): with d = dot(n, u), uu = dot(u, u) eligible when
 *               d d >= (cos2_tilt nn) uu; cos2_tilt = cos^2 of the largest tilt, evaluated in float64 and rounded once.
 *   inlier      s = dot(p - p0, n); s s <= (t t) nn, inclusive, t = threshold.
 *   winner      the valid eligible hypothesis with the most inliers, ties to the lower h; fewer than 3 inliers: no plane.
 * Outputs, all DEVICE memory, written whole (no host read, no synchronisation, no allocation):
 *   hypotheses (H,8) float32: n (3), p0 (3), nn, flag (0 invalid, 1 valid but gated out, 2 valid and eligible)
 *   counts     (H) int32: the inlier count of every flag-2 hypothesis, -1 for the others
 *   inlier     (M) uint8: 1 for the winner's inliers (all 0 without a plane)
 *   moments    (10) float64 over the winner's inliers, coordinates widened from float32: n, Sx, Sy, Sz, Sxx, Sxy, Sxz, Syy,
 *              Syz, Szz.  Float64 atomics: the order of the additions is not fixed -- the one non-bitwise output.
 *   winner     (2) int32: the winning h (or -1) and its count (or 0)
 *   workspace  regnet_plane_workspace_bytes(M, H) = 32 H bytes, 16-byte aligned (the count kernel's parameter rows); -1 for
 *              unsupported sizes.  hypotheses must be 16-byte aligned too.
 *   stages     15 = all four launches.  Bits 1 / 2 / 4 / 8 = hypotheses / counts / selection / mask + moments on their own,
 *              each reading what the earlier ones left in the outputs: for measurements.
 * Four launches ordered by the stream; no workgroup waits for another.  M == 0: every hypothesis invalid (zero rows, counts
 * -1), winner -1, moments 0; xyz / inlier may be NULL.  Errors, all before any launch: M < 0, H <= 0, H % 64 != 0 or stages
 * outside 1..15 -> REGNET_ERR_SHAPE; M > 2^21 or H > 4096 -> REGNET_ERR_UNSUPPORTED; a NULL pointer for a required array ->
 * REGNET_ERR_NULL.                                                                                                        */
int64_t regnet_plane_workspace_bytes(int64_t M, int64_t H);
int regnet_plane_estimate_f32(const float* xyz, int64_t M, int64_t H, uint64_t seed, float threshold, float range_lo,
                              float range_hi, const float* up_hint, float cos2_tilt, float* hypotheses, int32_t* counts,
                              uint8_t* inlier, double* moments, int32_t* winner, void* workspace, int stages, void* stream);
int regnet_plane_estimate_f64(const double* xyz, int64_t M, int64_t H, uint64_t seed, float threshold, float range_lo,
                              float range_hi, const float* up_hint, float cos2_tilt, float* hypotheses, int32_t* counts,
                              uint8_t* inlier, double* moments, int32_t* winner, void* workspace, int stages, void* stream);

/* regnet_plane_moments_det_f32 / _f64: the ten moments of the rows whose `inlier` byte is non-zero (and whose float32 coordinates
 * are finite), summed in ONE fixed order -- per 2048-point tile in the moments kernel's own order, the tiles' partial rows in
 * ascending order by one workgroup --, so two estimates of the same cloud give the same bits (the atomics of
 * regnet_plane_estimate_* do not).  moments (10) float64 DEVICE, written whole; workspace
 * regnet_plane_moments_det_workspace_bytes(M) = 80 max(1, ceil(M / 2048)) bytes, 8-byte aligned (-1 for M < 0 or M > 2^21).
 * Two launches, no atomics, no host read.  M == 0: zeros.  Errors as regnet_plane_estimate_*.                              */
int64_t regnet_plane_moments_det_workspace_bytes(int64_t M);
int regnet_plane_moments_det_f32(const float* xyz, int64_t M, const uint8_t* inlier, double* moments, void* workspace, void* stream);
int regnet_plane_moments_det_f64(const double* xyz, int64_t M, const uint8_t* inlier, double* moments, void* workspace, void* stream);

/* ---- depth frames (csrc/depth.hip): a depth image and an optional colour image -> the organised cloud, on the device ----------
 * regnet_depth_to_cloud_u16 / _f32: depth (H, W) contiguous, uint16 raw units or float32 metres; pixel (u, v) = column u, row v,
 * output row v W + u.  Pinhole intrinsics, no distortion model.  Canonical fp32 arithmetic: individually rounded binary32
 * operations in the written order (-ffp-contract=off); constants are evaluated in float64 by the caller and rounded once.
 *   params      (25) float32 HOST memory: rfx = float32(1 / fx), rfy, cx, cy, s (depth scale), lo, hi, t (edge threshold),
 *               margin, fxc, fyc, cxc, cyc, R (9, row-major), tr (3).  Entries a mode does not use are ignored.
 *   depth       uint16 d: z = float32(d) * s, d == 0: no depth.  float32: z = d; not finite or z <= 0: no depth.
 *               valid0 = has depth and lo <= z <= hi (inclusive), else status 0 / 1.
 *   edge filter use_edge != 0: a valid0 pixel is removed (status 2) when for one of its 8 neighbours q inside the image and valid0
 *               fabsf(z - zq) > t * fminf(z, zq) (strict).  Decided on valid0 alone, one pass: both sides of a jump lose a pixel.
 *               min_neighbours k in 0..8: fewer than k valid0 8-neighbours inside the image -> removed (status 3).
 *   deproject   x = ((float32(u) - cx) * z) * rfx, y = ((float32(v) - cy) * z) * rfy, z.  No division.
 *   colour      mode 0 (none): rgb = 0.  mode 1 (aligned): colour (H, W, 3) uint8 (Wc = W, Hc = H), rgb[k] = LUT[c[k]],
 *               LUT[i] = float32(i / 255.0) (regnet_depth_colour_lut writes the 256 entries to HOST memory).
 *               mode 2 (registered): colour (Hc, Wc, 3) uint8, Wc Hc <= 2^23.  p' = R p + tr with x' = ((r00 x + r01 y) + r02 z)
 *               + t0 and likewise y', z'; outside (status 4) when z' is not finite or z' <= 0; uc = (x' / z') * fxc + cxc with
 *               the correctly rounded division, fu = floorf(uc + 0.5f), inside when fu >= 0 && fu < Wc in float; likewise fv.
 *               Visibility: a uint32 z-buffer over the colour grid starts at the bits of +inf; every point that survived the
 *               filter and is inside does an unsigned atomicMin with the bits of z' into every pixel of the (2 splat + 1)^2
 *               footprint around (fu, fv) that lies in the image (splat 0..2); a point is visible when
 *               z' - zmin(fu, fv) <= margin (inclusive), else status 5.  A visible point takes LUT[colour(fv, fu)].
 *               keep_uncoloured != 0: status 4 / 5 rows keep their coordinates (rgb = 0); otherwise they are dropped.
 * Outputs, all DEVICE memory, written whole (no host read, no synchronisation, no allocation: capturable):
 *   xyz (H W, 3), rgb (H W, 3) float32; status (H W) uint8: 0 no depth, 1 out of range, 2 edge jump, 3 too few neighbours,
 *   4 outside the colour image, 5 occluded, 6 kept (the first that applies); counts (8) int32: the histogram of status.
 *   A row that is not kept holds the quiet NaN 0x7FC00000 in its three coordinates and rgb = 0.
 *   workspace   regnet_depth_workspace_bytes(W, H, Wc, Hc, mode): the z-buffer, 4 Wc Hc rounded up to 16, 16-byte aligned, in
 *               mode 2; 16 (not touched, may be NULL) otherwise; -1 for unsupported sizes.
 * Modes 0 / 1: a one-workgroup fill of counts and ONE launch (32 x 8 pixel tiles, depths + halo staged in LDS).  Mode 2: z-buffer
 * fill, points + atomicMin, colour -- three launches ordered by the stream; no workgroup waits for another.  Errors, all before
 * any launch: W < 1, H < 1, mode outside 0..2, (Wc, Hc) != (W, H) in mode 1 or < 1 in mode 2, min_neighbours outside 0..8,
 * splat outside 0..2 -> REGNET_ERR_SHAPE; W H > 2^21 or Wc Hc > 2^23 -> REGNET_ERR_UNSUPPORTED; a NULL pointer for a required
 * array -> REGNET_ERR_NULL.                                                                                                */
int64_t regnet_depth_workspace_bytes(int64_t W, int64_t H, int64_t Wc, int64_t Hc, int mode);
int regnet_depth_colour_lut(float* lut);
int regnet_depth_to_cloud_u16(const uint16_t* depth, int64_t W, int64_t H, const float* params, const uint8_t* colour, int64_t Wc,
                              int64_t Hc, int mode, int use_edge, int min_neighbours, int splat, int keep_uncoloured, float* xyz,
                              float* rgb, uint8_t* status, int32_t* counts, void* workspace, void* stream);
int regnet_depth_to_cloud_f32(const float* depth, int64_t W, int64_t H, const float* params, const uint8_t* colour, int64_t Wc,
                              int64_t Hc, int mode, int use_edge, int min_neighbours, int splat, int keep_uncoloured, float* xyz,
                              float* rgb, uint8_t* status, int32_t* counts, void* workspace, void* stream);

/* regnet_depth_normals_f32: the normals of an organised cloud from its own pixel grid (csrc/depth.hip), what the projective mode
 * of the pose refinement below takes.  xyz (H W, 3) float32 DEVICE, row v W + u for pixel (u, v), NaN rows for removed pixels
 * (regnet_depth_to_cloud_*'s output, or any cloud laid out like it).  A lane per pixel, individually rounded binary32 operations in
 * the written order.  Per pixel with a finite centre c:
 *   neighbour   the pixel `step` columns (rows) to either side is valid when it is inside the image, its three coordinates are
 *               finite and fabsf(z_nb - z_c) <= float32(max_jump) (inclusive): a difference never spans a depth discontinuity.
 *   h           along the image row: R - L (per coordinate) when both neighbours are valid, else R - c, else c - L, else the
 *               pixel has no normal.  g along the column the same way, D - U with v + step down.
 *   normal      n = h x g = ((h_y g_z) - (h_z g_y), (h_z g_x) - (h_x g_z), (h_x g_y) - (h_y g_x)); len2 = ((n_x n_x) + (n_y n_y))
 *               + (n_z n_z); not finite or <= 0: no normal.  Else every component is divided (correctly rounded) by the
 *               correctly rounded sqrtf(len2), and n is negated when ((n_x c_x) + (n_y c_y)) + (n_z c_z) > 0: it faces the
 *               camera at the origin.
 * normals (H W, 3) float32 DEVICE, written whole: a pixel without a normal -- a NaN centre included -- holds three quiet NaNs.
 * One launch, no host read, no synchronisation, no allocation: capturable.  Errors, all before the launch: W < 1, H < 1 or
 * step < 1 -> REGNET_ERR_SHAPE; W H > 2^21, max_jump not finite or not positive in float32 -> REGNET_ERR_UNSUPPORTED; a NULL
 * pointer -> REGNET_ERR_NULL.  (A step beyond the image leaves every pixel without a normal.)                               */
int regnet_depth_normals_f32(const float* xyz, int64_t W, int64_t H, int64_t step, double max_jump, float* normals, void* stream);

/* regnet_depth_bilateral_f32 / regnet_depth_halve_f32: the frame's side of a coarse-to-fine registration (csrc/depth.hip) -- the
 * edge-preserving smoothing of a depth image and one level of its pyramid.  depth (H, W) float32 DEVICE, metres; "no depth" on
 * input is a value that is not finite or <= 0, on output the quiet NaN 0x7FC00000.  Individually rounded binary32 operations in
 * the written order; the correctly rounded division.
 * regnet_depth_bilateral_f32: out (H, W).  radius r in 1..4.
 *   tables      ((2 r + 1)^2 + 256) float32 DEVICE, made by the caller in float64 and rounded once per entry: the spatial weights
 *               S[b][a] = float32(exp(-0.5 (a^2 + b^2) / sigma_space^2)), a, b = -r..r, row-major (b outer), then the range table
 *               G[i] = float32(exp(-0.5 (3 (i + 0.5) / 256)^2)), i = 0..255: three sigma_depth in 256 bins.  The kernel takes them
 *               as data and evaluates no exponential.
 *   rbin        float32(256 / (3 sigma_depth)), the division in float64: bins per metre.
 *   pixel       with a valid centre z_c: sw = sd = 0; for b = -r..r (outer), a = -r..r (inner), the centre in its place, every
 *               neighbour q = (u + a, v + b) inside the image and valid: d = z_q - z_c, t = fabsf(d) * rbin; when !(t < 256.0f) q
 *               is skipped (no weight beyond three sigma: nothing bleeds across a depth edge); else w = S[b][a] * G[(int)t],
 *               sw = sw + w, sd = sd + (w * d).  out = z_c + (sd / sw); sw >= S[0][0] G[0] > 0.  An invalid centre: NaN -- holes
 *               are not filled.
 *   One launch: a lane per pixel, 32 x 8 tiles, the halo of r pixels and both tables staged in LDS.  Errors, all before the
 *   launch: W < 1, H < 1 or radius outside 1..4 -> REGNET_ERR_SHAPE; W H > 2^21, rbin not finite or not positive in float32 ->
 *   REGNET_ERR_UNSUPPORTED; a NULL pointer -> REGNET_ERR_NULL.
 * regnet_depth_halve_f32: out (H / 2, W / 2) by integer division; an odd last column or row is dropped.
 *   block       coarse pixel (u, v) reads (2u, 2v), (2u + 1, 2v), (2u, 2v + 1), (2u + 1, 2v + 1), in that order.
 *   members     z_ref = the smallest valid depth of the four (the foreground wins; the rule is symmetric); a valid pixel is a
 *               member when z - z_ref <= float32(cutoff) (inclusive).
 *   out         (the sum of the members in block order, from 0) / float32(count); NaN without a valid pixel.
 *   A coarse pixel u is the ray through fine coordinate 2u + 0.5 (pixel centres sit at integers): the caller halves the
 *   intrinsics as fx / 2, fy / 2, (cx - 0.5) / 2, (cy - 0.5) / 2, in float64.
 *   One launch, a lane per coarse pixel.  Errors, all before the launch: W < 2 or H < 2 -> REGNET_ERR_SHAPE; W H > 2^21, cutoff
 *   not finite or not positive in float32 -> REGNET_ERR_UNSUPPORTED; a NULL pointer -> REGNET_ERR_NULL.
 * Both: no host read, no synchronisation, no allocation: capturable.  out must not alias depth.                              */
int regnet_depth_bilateral_f32(const float* depth, int64_t W, int64_t H, int64_t radius, const float* tables, double rbin,
                               float* out, void* stream);
int regnet_depth_halve_f32(const float* depth, int64_t W, int64_t H, double cutoff, float* out, void* stream);

/* ---- object segmentation (csrc/cluster.hip): Euclidean cluster extraction over one cloud, on the device --------------------
 * regnet_cluster_points_f32: xyz (N,3) float32 contiguous; mask (N) uint8 or NULL.  Canonical fp32 arithmetic: individually
 * rounded binary32 operations in the written order (-ffp-contract=off).
 *   graph rows  row i is in the graph iff (mask == NULL or mask[i] != 0) and its three coordinates are finite.  The other rows
 *               are compacted away before the uniform grid (csrc/grid.h) is built; they never reach it.
 *   edges       i ~ j iff d2 <= T2 (inclusive), d2 = ((dx dx) + (dy dy)) + (dz dz) with dx = x_i - x_j, T2 = tolerance * tolerance
 *               (one float32 product).  Symmetric by construction.  The grid visits the cells overlapping the ball; it only
 *               decides which pairs are evaluated.
 *   root        (N) int32: the smallest row of i's connected component, -1 for a row outside the graph -- independent of the
 *               order in which the atomics land.
 *   key         (N) int32: key[r] = the size of the component whose root is r when that size is >= min_points (the component
 *               is KEPT), 0 for every other row.
 *   ranking     kept components by descending size, equal sizes by smaller root; rank r < max_objects is object r.  The caller
 *               ranks between the two stages: order = the indices of a STABLE DESCENDING sort of key (its index is the root),
 *               of which the first min(N, max_objects) entries are read.  Entries outside [0, N) or with key 0 are no object.
 *   label       (N) int32: the object id, -1 for rows outside the graph, in dropped components or ranked >= max_objects.
 *   num         (2) int32 DEVICE: num[0] = min(kept, max_objects), num[1] = kept.
 *   object_size / object_first (max_objects) int32, object_bbox (max_objects,6) float32: size, root and (min x, y, z, max x, y,
 *               z) of the member coordinates for ids < num[0]; -1 / -1 / the quiet NaN 0x7FC00000 beyond.  min / max are exact,
 *               under the total order in which -0.0 < +0.0.
 *   stages      1: init + compaction, grid build, union, flatten + sizes, keys -> root, key.  2: tables, labels + boxes, box
 *               decode -> label, num, object_*; reads root, key, order and the workspace stage 1 left.  3: both, with `order`
 *               already in place (a re-run).  Outputs of a stage that does not run may be NULL.
 *   workspace   regnet_cluster_workspace_bytes(N, max_objects), 16-byte aligned: counters, the compacted rows and their source
 *               rows, the parent array, root -> object id, the grid slab; -1 for unsupported sizes.
 * Union: a thread per graph row unites with every in-tolerance row of higher index -- lock-free union-find on an int32 parent
 * array, the larger root hooked under the smaller by atomicCAS, paths halved by atomicMin.  Parent pointers only ever decrease,
 * every loop ends on its own and no thread waits for another workgroup.  No host read, no synchronisation, no allocation.
 * N == 0: success; stage 2 writes num = (0, 0) and the empty tables.  Errors, all before any launch: N < 0, min_points < 1,
 * max_objects < 1 or stages outside 1..3 -> REGNET_ERR_SHAPE; tolerance not finite or <= 0, N >= 2^31 or max_objects > 2^28 ->
 * REGNET_ERR_UNSUPPORTED (regnet_cluster_workspace_bytes: -1 for the same sizes); a NULL pointer for a required array ->
 * REGNET_ERR_NULL.  A failed launch or fill returns the positive hipError_t, as every launching entry point does.
 *
 * regnet_cluster_assign_f32: query (Q,3), xyz (N,3) float32 contiguous, label (N) int32.  point[q] = the row with label >= 0
 * and d2 <= R2 (inclusive; the same d2 with x_i the query; R2 = radius * radius, one float32 product) that is smallest by
 * (d2, row); object[q] = label[point[q]]; both -1 when there is none or the query has a non-finite coordinate.  A wave per
 * query over all N rows, one launch.  Q == 0: success.  Errors: Q < 0 or N < 0 -> REGNET_ERR_SHAPE; radius < 0 or NaN, Q or
 * N >= 2^31 -> REGNET_ERR_UNSUPPORTED; NULL -> REGNET_ERR_NULL.                                                            */
int64_t regnet_cluster_workspace_bytes(int64_t N, int64_t max_objects);
int regnet_cluster_points_f32(const float* xyz, const uint8_t* mask, int64_t N, float tolerance, int64_t min_points,
                              int64_t max_objects, int32_t* root, int32_t* key, const int64_t* order, int32_t* label,
                              int32_t* num, int32_t* object_size, int32_t* object_first, float* object_bbox, void* workspace,
                              int stages, void* stream);
int regnet_cluster_assign_f32(const float* query, int64_t Q, const float* xyz, const int32_t* label, int64_t N, float radius,
                              int32_t* object, int32_t* point, void* stream);

/* ---- outlier removal (csrc/outlier.hip): radius and statistical cloud filters over one cloud, on the device -------------------
 * xyz (N,3) float32 contiguous; mask (N) uint8 or NULL.  Canonical fp32 arithmetic: individually rounded binary32 operations in
 * the written order (-ffp-contract=off).
 *   graph rows  row i is in the graph iff (mask == NULL or mask[i] != 0) and its three coordinates are finite.  The other rows
 *               are compacted away before the uniform grid (csrc/grid.h) is built; the count of graph rows stays on the device.
 *   distance    d2 = ((dx dx) + (dy dy)) + (dz dz); j is within range of i iff d2 <= R2 (inclusive), R2 = R * R (one float32
 *               product).  The grid's cell edge starts at R and coarsens under its cell limit; the walk visits the cells
 *               overlapping the ball, and only decides which pairs are evaluated.
 * regnet_outlier_radius_f32: n(i) = the graph rows j != i within `radius` of i, compared by ROW (a duplicate point counts).
 *   count       (N) int32: min(n(i), min_neighbours); -1 for a row outside the graph.  A row is an inlier iff count[i] ==
 *               min_neighbours (open3d's remove_radius_outlier: the neighbours found, the point itself among them, exceed
 *               nb_points).  A row's walk stops as soon as it has min_neighbours.
 * regnet_outlier_knn_f32: among the graph rows j != i within `max_radius`, the k smallest d2 (1 <= k <= 64; ties need no rule,
 *   only the multiset of values is used).
 *   found       (N) int32: min(n(i), k); -1 for a row outside the graph.
 *   mean_dist   (N) float32: where found == k, float32(S / k) with S the float64 sum of the correctly rounded float32 sqrt(d2)
 *               taken in ascending order of d2, one addition after the other, and a float64 division; the quiet NaN 0x7FC00000
 *               elsewhere.  Independent of the order in which candidates are met: two runs give the same bytes.
 * regnet_outlier_stats_f64: over the rows with found == k, in float64 and a fixed order (one workgroup: thread t of 1024 adds
 *   rows t, t + 1024, ... one after the other, then a binary tree over the threads):
 *   stats       (4) float64 DEVICE = n, mu = sum(m) / n, sigma = sqrt(sum((m - mu)^2) / (n - 1)) in a second pass (open3d's
 *               form), thr = float32(mu + ratio * sigma) stored as a double.  n < 2: sigma = NaN, thr = +inf; n == 0: mu = NaN.
 *               A row passes the statistical filter iff mean_dist <= thr (a NaN fails).
 *   workspace   regnet_outlier_workspace_bytes(N), 16-byte aligned: a counter, the compacted rows and their source rows, the
 *               grid slab; -1 for unsupported sizes.
 * No host read, no synchronisation, no allocation.  Errors, all before any launch: N < 0 -> REGNET_ERR_SHAPE; N >= 2^31, k
 * outside 1..64, min_neighbours < 1, a radius that is not positive and finite, a ratio that is negative or not finite ->
 * REGNET_ERR_UNSUPPORTED; a NULL pointer for a required array -> REGNET_ERR_NULL.  N == 0: success, the radius and knn entries
 * touch no output (the statistics are those of no row).                                                                       */
int64_t regnet_outlier_workspace_bytes(int64_t N);
int regnet_outlier_radius_f32(const float* xyz, const uint8_t* mask, int64_t N, float radius, int64_t min_neighbours,
                              int32_t* count, void* workspace, void* stream);
int regnet_outlier_knn_f32(const float* xyz, const uint8_t* mask, int64_t N, int64_t k, float max_radius, float* mean_dist,
                           int32_t* found, void* workspace, void* stream);
int regnet_outlier_stats_f64(const float* mean_dist, const int32_t* found, int64_t N, int64_t k, double ratio, double* stats,
                             void* stream);

/* ---- multi-view fusion (csrc/fuse.hip): a voxel-grid merge of up to 8 posed clouds into one cloud, on the device ------------
 * One output point per occupied voxel: the centroid of the voxel's points and colours.  Canonical fp32 arithmetic: individually
 * rounded binary32 operations in the written order (-ffp-contract=off); no float is ever summed, so the result is bitwise
 * reproducible and independent of the order in which the atomics land.
 *   rows        view v has n_v rows: xyz (n_v,3) float32 contiguous, rgb (n_v,3) float32 contiguous or NULL (colour 0).  The
 *               global row of row r of view v is row_offset_v + r, row_offset_v = n_0 + ... + n_{v-1} (the caller's sum).  A row
 *               whose three coordinates are not all finite is dropped and counted.
 *   pose        pose12 (12 float32, HOST): rows 0..2 of the row-major 4x4 camera-to-common transform, each entry rounded once
 *               from float64 by the caller.  x' = ((r00 x + r01 y) + r02 z) + t0 and likewise y', z'.
 *   voxel       inv = float32(1.0 / voxel), the division in float64; origin3 (3 float32, HOST).  Per axis a = (x' - ox) * inv,
 *               i = floorf(a), f = a - float32(i) (in [0, 1]; 1 only where a tiny negative a rounds up).  A row whose a is not
 *               finite or whose i lies outside [-2^20, 2^20) on any axis is out of range: dropped and counted.
 *   key         ((ix + 2^20) << 42) | ((iy + 2^20) << 21) | (iz + 2^20), uint64, below 2^63; all ones marks an empty slot.
 *   table       regnet_fuse_table_slots(max_voxels) = 2 * next_pow2(max_voxels) slots, open addressing with linear probing; the
 *               home slot is the top log2(slots) bits of key * 0x9E3779B97F4A7C15 (mod 2^64).  A row claims an empty slot with a
 *               64-bit atomicCAS on the key word.  The probe loop is bounded by the slot count.  A row that finds no slot, or
 *               that opens voxel number max_voxels + 1 or a later one, sets the overflow flag and is dropped.
 *   per slot    count: int32 add; S_x, S_y, S_z: 64-bit adds of (int32)(f * 16777216.0f); C_r, C_g, C_b: 64-bit adds of
 *               (int32)rintf(clamp(c, 0, 1) * 255.0f), a NaN colour counting as 0; first: atomicMin of the global row; views:
 *               atomicOr of 1 << view.
 *   output      voxels with count >= min_count, in ascending key order, K of them.  count == 1: the transformed point (x', y', z')
 *               of row `first` and its colour as given, bit for bit.  Otherwise, in float64 with one rounding per operation:
 *               a_mean = i + S / (count * 2^24), x = float32(ox + a_mean / (double)inv); colour = float32(C / (count * 255.0)).
 *   xyz, rgb    (max_voxels,3) float32: rows >= K hold the quiet NaN 0x7FC00000 / 0.
 *   count, views, first  (max_voxels) int32: -1 for rows >= K.
 *   num         (4) int32 DEVICE: K, rows accumulated into a voxel, rows dropped (non-finite + out of range), overflow 0 / 1.
 *               With overflow set the rows are a merge of a subset of the input and num[1] + num[2] is below the row count.
 * The three stages of one merge share `workspace`: regnet_fuse_workspace_bytes(max_voxels) bytes, 16-byte aligned (64 bytes of
 * counters, 92 bytes per slot, 4 bytes per voxel); -1 for max_voxels outside [1, 2^21], as regnet_fuse_table_slots.
 *   regnet_fuse_accumulate_f32  stage 1 for ONE view, called once per view on the same workspace, view = 0..7.  reset != 0 first
 *               empties the table and the counters (three fills); give it on the first call of a merge.  n == 0: success, and
 *               with reset the table is still emptied.  One launch, a thread per row.
 *   regnet_fuse_finalise_f32    stage 2: kept_keys (max_voxels) int64 DEVICE is written whole: the keys of the kept voxels in
 *               its first K entries, in any order, 0x7FFFFFFFFFFFFFFF beyond.  Two launches.
 *   (the caller)                order = the indices of an ascending sort of kept_keys (the keys are distinct).
 *   regnet_fuse_emit_f32        stage 3: order (max_voxels) int64 DEVICE, of which the first K entries are read; writes the
 *               outputs whole.  One launch.
 * No host read, no synchronisation, no allocation; no thread waits for another and every loop ends on its own count.  Errors,
 * all before any launch: n < 0, row_offset < 0, view < 0 or min_count < 1 -> REGNET_ERR_SHAPE; view >= 8, voxel not finite or
 * <= 0, max_voxels outside [1, 2^21] or row_offset + n >= 2^31 -> REGNET_ERR_UNSUPPORTED; a NULL pointer for a required array ->
 * REGNET_ERR_NULL.
 *
 * HOST code, no device: regnet_fuse_key_host evaluates pose, voxel and key of one point with the inline functions the kernel is
 * compiled from -> 0 and *key; 1 (a non-finite coordinate) or 2 (out of range) and *key = all ones.  regnet_fuse_home_slot_host:
 * the home slot of `key` in a table of `slots` slots (a power of two in [2, 2^22], else -1).                                  */
int64_t regnet_fuse_table_slots(int64_t max_voxels);
int64_t regnet_fuse_workspace_bytes(int64_t max_voxels);
int regnet_fuse_key_host(float x, float y, float z, const float* pose12, const float* origin3, float inv, uint64_t* key);
int64_t regnet_fuse_home_slot_host(uint64_t key, int64_t slots);
int regnet_fuse_accumulate_f32(const float* xyz, const float* rgb, int64_t n, int view, int64_t row_offset, const float* pose12,
                               const float* origin3, double voxel, int64_t max_voxels, int reset, void* workspace, void* stream);
int regnet_fuse_finalise_f32(int64_t max_voxels, int64_t min_count, int64_t* kept_keys, void* workspace, void* stream);
int regnet_fuse_emit_f32(const int64_t* order, const float* origin3, double voxel, int64_t max_voxels, float* xyz, float* rgb,
                         int32_t* count, int32_t* views, int32_t* first, int32_t* num, void* workspace, void* stream);

/* ---- TSDF volume (csrc/tsdf.hip): depth views fused into a truncated signed distance volume, its surface extracted -----------
 * Voxel-parallel, one owner per voxel: no floating-point atomic and no sum whose order is open.  Canonical fp32 arithmetic:
 * individually rounded binary32 operations in the written order (-ffp-contract=off), divisions correctly rounded (__fdiv_rn),
 * roots correctly rounded (sqrtf).  voxel_f = float32(voxel), trunc_f = float32(trunc), rtrunc = float32(1.0 / trunc) with the
 * division in float64; origin3 (3 float32, HOST), rounded once by the caller.
 *   volume      nx x ny x nz voxels, N = nx ny nz <= 2^28; the linear index of voxel (ix, iy, iz) is l = (iz ny + iy) nx + ix.
 *               `volume` is FIVE PLANES of N 4-byte words, 20 bytes per voxel, 4-byte aligned: D (N float32, the running mean of
 *               the truncated distance in units of trunc), W (N int32, the observation count), C_r, C_g, C_b (N float32 each, the
 *               running mean colour).  Planes and not interleaved records: a wave of 64 consecutive ix then reads and writes 256
 *               contiguous bytes of every plane, and the extraction, which needs D and W only, leaves the colours in HBM.
 *               regnet_tsdf_bytes(nx, ny, nz) = 20 N, -1 for dims < 1 or N > 2^28.  regnet_tsdf_integrate_workgroups: the
 *               workgroups of one integrate launch for these dims (the tiling below), -1 likewise; tests size a case by it.
 *   centre      p_k = o_k + ((float)i_k + 0.5f) * voxel_f per axis k.
 * regnet_tsdf_reset: D = 1, W = 0, C = 0 for every voxel.  One launch.
 * regnet_tsdf_integrate_f32: ONE view into the volume; the views' order is the call order and is part of the result.
 *   xyz         (height width, 3) float32: the view's organised cloud in ITS CAMERA's frame, row v width + u for pixel (u, v), a
 *               row without a point holding a non-finite z (regnet_depth_to_cloud_*'s output); only z is read.
 *   rgb         (height width, 3) float32 or NULL (colour 0).
 *   intrinsics4 (4 float32, HOST): fx, fy, cx, cy.   pose12 (12 float32, HOST): rows 0..2 of the row-major 4x4 COMMON-TO-CAMERA
 *               transform, inverted in float64 by the caller and rounded once.
 *   per voxel   1. x = (((r00 px) + (r01 py)) + (r02 pz)) + t0 and likewise y, z.  z not finite or z <= 0: NOT IN VIEW.
 *               2. u = (__fdiv_rn(x, z) * fx) + cx, fu = floorf(u + 0.5f); inside iff fu >= 0 && fu < (float)width, compared in
 *                  float (a NaN fails); likewise v with fy, cy, height.  Outside: NOT IN VIEW.  (regnet_depth_to_cloud_*'s
 *                  projection, restated.)
 *               3. zd = xyz[(fv width + fu) 3 + 2].  Not finite: NO DEPTH.
 *               4. sdf = zd - z.  sdf < -trunc_f: BEHIND the surface, the voxel is untouched.  Else t = fminf(sdf * rtrunc, 1.0f).
 *               5. Wf = (float)W;  D = __fdiv_rn((D * Wf) + t, Wf + 1.0f);  C_c = __fdiv_rn((C_c * Wf) + rgb_c, Wf + 1.0f) for
 *                  the pixel's colour (0 with rgb NULL);  W = min(W + 1, max_weight).  UPDATED.
 *   counts      (4) int32 DEVICE, this call's histogram: updated, not in view, no depth, behind (their sum is N).  Cleared by a
 *               one-workgroup kernel, then one integer atomic per workgroup and code.
 *               Two launches.  A 64 x 4 tile of voxels per 256-thread workgroup, ix on the lane, over 16 z layers one after the
 *               other.  A layer of the tile none of whose voxels is in view (decided by step 1-2 of every one of them) only adds
 *               its voxel count to the not-in-view code; a workgroup all of whose layers are so never touches the volume.
 * Extraction.  A candidate is (voxel v, axis a in 0..2 = x, y, z) whose neighbour n = v + e_a is inside the volume.  It is kept iff
 *               W_v >= min_weight && W_n >= min_weight, D_v < 1 && D_n < 1, and (D_v < 0) != (D_n < 0).  Its key is 3 l(v) + a.
 *   row         s = __fdiv_rn(D_v, D_v - D_n).  xyz = p_v with (p_v[a] + (s * voxel_f)) on axis a.  rgb_c = C_v + (s * (C_n - C_v)).
 *               gradient of a voxel q along axis k, with lo = q - e_k, hi = q + e_k `usable` iff inside and W >= min_weight:
 *               both: D(hi) - D(lo); hi only: (D(hi) - D(q)) * 2.0f; lo only: (D(q) - D(lo)) * 2.0f; neither: 0.
 *               g_k = gv_k + (s * (gn_k - gv_k)); len2 = ((gx gx) + (gy gy)) + (gz gz); len2 finite and > 0: normal_k =
 *               __fdiv_rn(g_k, sqrtf(len2)), else three quiet NaNs.  D grows towards free space: the normal points out of the
 *               surface.  weight = min(W_v, W_n).
 *   regnet_tsdf_count   pass 1: block_counts (regnet_tsdf_blocks(nx, ny, nz) = ceil(N / 256)) int32 DEVICE, the kept candidates
 *               of the voxels l in [256 b, 256 b + 256); num[2] = the voxels with W >= min_weight (num is cleared first).  Two
 *               launches; a workgroup takes 16 blocks one after the other and adds to num[2] once.
 *   (the caller)        block_base = the exclusive prefix sum of block_counts, int32 DEVICE.
 *   regnet_tsdf_emit_f32  pass 2: recomputes the predicate, ranks the kept candidates of a workgroup in key order (ballots within a
 *               wave, the waves' totals through LDS) and writes row block_base[b] + rank when that is below max_points: rows
 *               ascend by key with no sort.  With T = block_base[last] + block_counts[last] and K = min(T, max_points):
 *               xyz, rgb, normal (max_points,3) float32 and weight (max_points) int32, rows >= K holding the quiet NaN
 *               0x7FC00000 / 0 / NaN / -1; num (4) int32 DEVICE = K, T, (pass 1's) voxels with W >= min_weight, overflow = T >
 *               max_points.  On overflow the rows are those of the max_points smallest keys.  Two launches.  num must be the
 *               array pass 1 was given.
 * No host read, no synchronisation, no allocation, no cooperative launch; no workgroup waits for another.  Errors, all before any
 * launch: a dim, width, height, max_weight, min_weight or max_points < 1 -> REGNET_ERR_SHAPE; N > 2^28, width height > 2^21,
 * max_points > 2^21, voxel or trunc not finite or not positive (in float32 too), 1 / trunc not finite in float32 ->
 * REGNET_ERR_UNSUPPORTED; a NULL pointer for a required array -> REGNET_ERR_NULL.                                          */
int64_t regnet_tsdf_bytes(int64_t nx, int64_t ny, int64_t nz);
int64_t regnet_tsdf_blocks(int64_t nx, int64_t ny, int64_t nz);
int64_t regnet_tsdf_integrate_workgroups(int64_t nx, int64_t ny, int64_t nz);
int regnet_tsdf_reset(void* volume, int64_t nx, int64_t ny, int64_t nz, void* stream);
int regnet_tsdf_integrate_f32(void* volume, int64_t nx, int64_t ny, int64_t nz, const float* origin3, double voxel, double trunc,
                              int64_t max_weight, const float* xyz, const float* rgb, int64_t width, int64_t height,
                              const float* intrinsics4, const float* pose12, int32_t* counts, void* stream);
int regnet_tsdf_count(const void* volume, int64_t nx, int64_t ny, int64_t nz, int64_t min_weight, int32_t* block_counts,
                      int32_t* num, void* stream);
int regnet_tsdf_emit_f32(const void* volume, int64_t nx, int64_t ny, int64_t nz, const float* origin3, double voxel,
                         int64_t min_weight, const int32_t* block_counts, const int32_t* block_base, int64_t max_points,
                         float* xyz, float* rgb, float* normal, int32_t* weight, int32_t* num, void* stream);

/* Triangle mesh (csrc/tsdf_mesh.hip): marching cubes over the extraction above.  The mesh's vertices ARE the rows of
 * regnet_tsdf_emit_f32; these entry points add the index buffer.  Integer work only: D < 0 and D < 1 are the only floating-point
 * operations, so nothing is rounded, and two runs give the same bytes.
 *   cell        addressed by the linear index l of its low corner voxel (ix, iy, iz), ix < nx - 1, iy < ny - 1, iz < nz - 1; any dim
 *               < 2: no cell, a valid empty mesh.  Corner c in 0..7 is voxel (ix + (c & 1), iy + (c >> 1 & 1), iz + (c >> 2 & 1)).  A
 *               corner is USABLE iff W >= min_weight && D < 1.0f (a NaN is not); a cell is MESHED iff all eight are.  Its case
 *               is the 8-bit mask of the corners with D < 0.0f (+0 and -0 are both outside).  Every sign-changing edge of a
 *               meshed cell is a kept candidate of the extraction: the mesh never needs a vertex the surface lacks.
 *   edge        of a cell: (corner c, axis a) with bit a of c clear, joining c to c | 1 << a; the twelve are numbered in ascending
 *               (c, a).  Its vertex is the surface row whose key is 3 l(voxel of c) + a.
 *   case table  256 cases, at most 5 triangles each, as edge numbers; derived (csrc/tsdf_mesh_table.h at compile time,
 *               tests/tsdf_mesh_reference.py in Python), not copied.  On each of the six faces (k, s) -- the corners whose bit k
 *               is s, in the cyclic order q0..q3 = (0,0), (1,0), (1,1), (0,1) of their (u, v) = ((k + 1) % 3, (k + 2) % 3) bits,
 *               face edge E_i joining q_i to q_(i+1) -- every maximal run q_i .. q_j of inside corners (not none, not all) is
 *               cut off by ONE segment from E_(i-1) to E_j: two diagonal inside corners are cut off one by one, by the face's
 *               own four signs, so two cells that share a face agree on it.  Seen from outside the cell a segment runs clockwise
 *               round its run (E_(i-1) -> E_j for s = 1, reversed for s = 0).  A crossed edge ends one segment and starts one:
 *               closed directed loops of 3 to 7 edges, in ascending order of their lowest edge.  Loop v_0 .. v_(n-1) becomes
 *               the fan (v_0, v_i, v_(i+1)), i = 1 .. n - 2, from the apex v_0: the loop's edge with the fewest fan diagonals
 *               that lie in a cube face (none for every loop of the 256 cases), the lowest edge number among equals.  The
 *               right-hand-rule normal of every triangle points towards D > 0, where the surface's normals point.  820
 *               triangles in all.  regnet_tsdf_mesh_case(case, edges16): HOST only, the compiled table's row -- three edge
 *               numbers per triangle, -1 in the unused slots --, REGNET_ERR_SHAPE for a case outside 0..255.
 *   order       triangles ascend by cell l and within a cell follow the table: no sort.
 *   regnet_tsdf_mesh_blocks(nx, ny, nz) = ceil(N / 256), the blocks of 256 consecutive l; regnet_tsdf_mesh_scratch_bytes = 4 N; -1
 *               each for dims < 1 or N > 2^28.
 *   regnet_tsdf_mesh_count   pass 1: tri_block_counts (regnet_tsdf_mesh_blocks) int32 DEVICE, the triangles of the cells l in
 *               [256 b, 256 b + 256); num_tri is cleared.  Two launches; a workgroup takes 16 blocks one after the other.
 *   (the caller)        tri_block_base = the exclusive prefix sum of tri_block_counts, int32 DEVICE (at most 5 N < 2^31).
 *   regnet_tsdf_mesh_emit    pass 2.  block_counts, block_base: the arrays regnet_tsdf_count left and the caller's prefix sum of
 *               them, and K_source: the num array regnet_tsdf_emit_f32 wrote (K = K_source[0] is read on the device), all of
 *               the SAME volume state and min_weight, enqueued before this call.  First the row lookup: the extraction's
 *               predicate is recomputed and ranked as pass 2 of the extraction ranks it, and every voxel with a kept candidate
 *               leaves (min(first row, 2^28 - 1) << 3) | kept axes in `scratch` (regnet_tsdf_mesh_scratch_bytes, 4-byte aligned,
 *               the caller's; the other words are neither written nor read): the row of candidate (v, a) is v's first row plus
 *               its kept axes below a.  Then the cells: the case is recomputed, the triangles of a block are ranked in cell
 *               order (ballots over the bits of the per-cell count, the waves' totals through LDS), and triangle row
 *               tri_block_base[b] + rank, when below max_triangles, receives its three vertex rows -- or (-1, -1, -1) IN ITS PLACE
 *               when one of them is >= K (the surface overflowed max_points), so ranks do not move.
 *   outputs     tri (max_triangles, 3) int32 DEVICE; with Tt = tri_block_base[last] + tri_block_counts[last] and Kt = min(Tt,
 *               max_triangles), rows >= Kt hold -1.  num_tri (4) int32 DEVICE = Kt, Tt, dropped (the rows < Kt written as
 *               (-1, -1, -1)), overflow = Tt > max_triangles; on overflow the rows are those of the smallest cells.  num_tri must
 *               be the array pass 1 was given.  Three launches.
 *   degenerate  D_v == 0 puts the vertices of up to three edges on one voxel centre: zero-area triangles, which are KEPT -- the
 *               mesh stays closed.  A cell with a corner that is not usable is not meshed: the mesh has holes along the border
 *               of observed space.
 * No host read, no synchronisation, no allocation, no cooperative launch, no floating-point arithmetic; capturable.  Errors, all
 * before any launch: a dim, min_weight or max_triangles < 1 -> REGNET_ERR_SHAPE; N > 2^28 or max_triangles > 2^22 ->
 * REGNET_ERR_UNSUPPORTED; a NULL pointer -> REGNET_ERR_NULL.                                                                  */
int64_t regnet_tsdf_mesh_blocks(int64_t nx, int64_t ny, int64_t nz);
int64_t regnet_tsdf_mesh_scratch_bytes(int64_t nx, int64_t ny, int64_t nz);
int regnet_tsdf_mesh_case(int64_t case_index, int8_t* edges16);
int regnet_tsdf_mesh_count(const void* volume, int64_t nx, int64_t ny, int64_t nz, int64_t min_weight, int32_t* tri_block_counts,
                           int32_t* num_tri, void* stream);
int regnet_tsdf_mesh_emit(const void* volume, int64_t nx, int64_t ny, int64_t nz, int64_t min_weight, const int32_t* block_counts,
                          const int32_t* block_base, const int32_t* K_source, const int32_t* tri_block_counts,
                          const int32_t* tri_block_base, int64_t max_triangles, void* scratch, int32_t* tri, int32_t* num_tri,
                          void* stream);

/* Mesh simplification (csrc/mesh_simplify.hip): vertex clustering (Rossignac-Borrel) of the mesh above, or of any mesh laid out
 * like it.  The vertices are merged per cell of a dense coarse grid -- the voxel merge of regnet_fuse_* applied to vertices --, the
 * index buffer is remapped, triangles that collapse leave and, with dedupe, equal triangles are made one.  Integer accumulation
 * only; the order of the grid is the order of the vertices and the order of the source rows that of the triangles: no sort, and two
 * runs give the same bytes whatever the order in which threads arrive.  Canonical arithmetic: every operation individually rounded
 * in the written order (-ffp-contract=off), __fdiv_rn.
 *   inputs      xyz, normal, rgb (rows, 3) float32 DEVICE: the vertex rows of a surface; K_source: its num, K = K_source[0] is read
 *               on the device (and held to 0..rows).  tri (max_tri_in, 3) int32 DEVICE and num_tri_in: the index buffer and num_tri
 *               of regnet_tsdf_mesh_emit, Kt = num_tri_in[0] is read on the device (and held to 0..max_tri_in); only the rows t < Kt
 *               are read.  origin3: 3 float32 on the HOST; cell: the edge of a grid cell, cell_f = (float)cell; the grid gx gy gz,
 *               each >= 1, G = gx gy gz <= 2^21; dedupe 0 / 1; max_vertices in 1..2^21, max_triangles in 1..2^22.
 *   cell        of a vertex, per axis: a = __fdiv_rn(x - o, cell_f), i = floorf(a), f = a - (float)i.  The vertex is VALID iff its
 *               three coordinates are finite and 0 <= i < g on every axis, its cell then c = (iz gy + iy) gx + ix; else STRAY.
 *   per cell    count (int32); S_k += (int32)(f_k * 16777216.0f), C_k += (int32)rintf(clamp(c_k, 0, 1) * 255.0f) (a NaN colour
 *               counts as 0), both 64-bit; a vertex whose three normal components are finite adds (int32)rintf(clamp(n_k, -1, 1) *
 *               1048576.0f) to N_k (64-bit) and 1 to ncount; first = the smallest vertex row (atomicMin).
 *   triangles   row t < Kt: (-1, -1, -1) is ABSENT; an index outside [0, K) or a STRAY vertex makes it STRAY; two equal cells among
 *               its three: COLLAPSED.  Otherwise the triple of cells is rotated cyclically until the smallest stands first -- the
 *               orientation is kept -- and key = c0 << 42 | c1 << 21 | c2.  With dedupe the rows of one key are one triangle: the
 *               SMALLEST source row survives, the others are DUPLICATE (an open-addressing set, linear probing from the home slot
 *               regnet_mesh_simplify_home_slot_host(key, slots) -- the top log2(slots) bits of key * 0x9E3779B97F4A7C15, as
 *               regnet_fuse_home_slot_host --, claimed by a 64-bit compare-and-swap, slots = regnet_mesh_simplify_table_slots =
 *               2 next_pow2(max_tri_in), so it cannot fill).  Two triangles of opposite orientation have different keys: both
 *               stay.  Without dedupe every row that is not COLLAPSED survives.
 *   vertices    the cells that a surviving triangle references, in ascending c: Kv of them, row < min(Kv, max_vertices) written.
 *               count == 1: position, normal and colour of row `first` as given, bit for bit.  Otherwise in float64, one rounding
 *               per operation: x = (float)(o + ((double)i + (double)S / ((double)count * 2^24)) * (double)cell_f); colour = (float)
 *               ((double)C / ((double)count * 255.0)); normal: m_k = (double)N_k / 1048576.0, len = sqrt((m_x m_x + m_y m_y) + m_z
 *               m_z), (float)(m_k / len), the quiet NaN 0x7fc00000 when ncount == 0 or len == 0.  out_weight = count.  The rows
 *               beyond hold NaN / NaN / 0 / -1 (xyz, normal, rgb, weight), as a surface's do.
 *   out_tri     (max_triangles, 3) int32: the survivors in ascending source row, each as its rotated triple in NEW vertex rows;
 *               -1 beyond the kept rows; a survivor with a vertex row >= max_vertices is (-1, -1, -1) IN ITS PLACE and dropped.
 *   num         (12) int32 DEVICE: [0] min(Kv, max_vertices), [1] Kv, [2] Kv > max_vertices, [3] cells with count > 0, [4] STRAY
 *               vertices, [5] min(Tt, max_triangles) with Tt the survivors, [6] Tt, [7] dropped (among the rows < [5]), [8] Tt >
 *               max_triangles, [9] COLLAPSED, [10] DUPLICATE, [11] STRAY + ABSENT; [6] + [9] + [10] + [11] = Kt.  Words 5..8 are a
 *               num_tri.  surface_num (4) int32 DEVICE or NULL: ([0], [1], K, [2]), the num of the new vertices as a surface.
 *   workspace   regnet_mesh_simplify_workspace_bytes(G, max_tri_in) bytes, 8-byte aligned (else REGNET_ERR_UNSUPPORTED), the
 *               caller's; -1 for sizes the call refuses.  Nothing in it outlives the call.
 * Two fills and eight launches on `stream`.  No sort, no host read, no synchronisation, no allocation, no cooperative launch; no
 * thread waits for another and every probe loop ends on the slot count; capturable.  K or Kt of 0: a valid empty mesh.  Errors, all
 * before any launch: rows, max_tri_in, a grid dim, max_vertices or max_triangles < 1, dedupe not 0 / 1 -> REGNET_ERR_SHAPE; G > 2^21,
 * rows or max_vertices > 2^21, max_triangles or max_tri_in > 2^22, cell not finite and positive (in float32 too) ->
 * REGNET_ERR_UNSUPPORTED; a NULL pointer (all but surface_num) -> REGNET_ERR_NULL.                                              */
int64_t regnet_mesh_simplify_workspace_bytes(int64_t G, int64_t max_tri_in);
int64_t regnet_mesh_simplify_table_slots(int64_t max_tri_in);
int64_t regnet_mesh_simplify_home_slot_host(uint64_t key, int64_t slots);
int regnet_mesh_simplify_f32(const float* xyz, const float* normal, const float* rgb, int64_t rows, const int32_t* K_source,
                             const int32_t* tri, int64_t max_tri_in, const int32_t* num_tri_in, const float* origin3, double cell,
                             int64_t gx, int64_t gy, int64_t gz, int dedupe, int64_t max_vertices, int64_t max_triangles,
                             void* workspace, float* out_xyz, float* out_normal, float* out_rgb, int32_t* out_weight,
                             int32_t* out_tri, int32_t* num, int32_t* surface_num, void* stream);

/* regnet_tsdf_raycast_f32: the MODEL VIEW of the volume from a virtual pinhole camera -- per pixel the first zero crossing of D
 * along its ray, with the normal of D's gradient and the colour there: the organised vertex and normal map
 * regnet_icp_step_projective_f32 takes as its target (frame-to-model tracking), and a denoised depth image of the fused model.
 * The volume is only read (D, W, and C when rgb is given).  A lane per pixel; the canonical fp32 arithmetic of the section above.
 *   volume, dims, origin3, voxel, min_weight   as for regnet_tsdf_emit_f32; here every dim <= 2^24 (the inside test below then
 *               compares exact floats).
 *   intrinsics4 (4 float32, HOST): rfx = float32(1 / fx), rfy = float32(1 / fy), cx, cy, the reciprocals taken in float64.
 *   pose12      (12 float32, HOST): rows 0..2 of the row-major 4x4 CAMERA-TO-COMMON transform, rounded once (not inverted).
 *   near, step, n_steps   the depth of sample i is z_i = near_f + ((float)i * step_f), i = 0 .. n_steps - 1; never accumulated.
 *   ray point   of pixel (u, v) at depth z.  Camera frame: c_x = (((float)u - cx) * z) * rfx, c_y = (((float)v - cy) * z) * rfy,
 *               c_z = z (regnet_depth_to_cloud_*'s deprojection).  Common frame: p_k = (((r_k0 c_x) + (r_k1 c_y)) + (r_k2 c_z)) + t_k.
 *   sample S(p) per axis g_k = __fdiv_rn(p_k - o_k, voxel_f) - 0.5f, i_k = floorf(g_k), f_k = g_k - i_k.  INSIDE iff for every axis
 *               i_k >= 0 && i_k + 1.0f <= (float)(n_k - 1), compared in float (a NaN fails).  KNOWN iff inside and the eight
 *               voxels (i_x + a, i_y + b, i_z + c), a, b, c in {0, 1}, all have W >= min_weight; else UNKNOWN.  The value of a
 *               plane P there: along x c_bc = P_0bc + (f_x * (P_1bc - P_0bc)), along y c_c = c_0c + (f_y * (c_1c - c_0c)), along z
 *               c_0 + (f_z * (c_1 - c_0)).  S is that value of D.
 *   march       over i ascending, with "previous" = the sample i - 1 when it was known with a value > 0 (a NaN value is none):
 *               an unknown sample: no previous.  A known sample with value v <= 0: with no previous the ray ends as BACK FACE (it
 *               came out of unseen space behind a surface, or started inside one); with the previous v_prev it ends as a HIT,
 *               s = __fdiv_rn(v_prev, v_prev - v), z_hit = z_{i-1} + (s * step_f).  Any other known sample becomes the previous
 *               when its value is > 0.  A ray that ends neither way: NO SURFACE.
 *   hit         xyz = the camera-frame ray point at z_hit; p = its common-frame point.
 *   normal      g_k = S(p + voxel_f e_k) - S(p - voxel_f e_k); any of the six unknown: HIT, NO NORMAL.  Into the camera frame with
 *               the transpose: n_x = ((r_00 g_x) + (r_10 g_y)) + (r_20 g_z), likewise n_y, n_z.  len2 = ((n_x n_x) + (n_y n_y)) +
 *               (n_z n_z); not finite or <= 0: HIT, NO NORMAL.  Else n_k = __fdiv_rn(n_k, sqrtf(len2)), negated when
 *               ((n_x c_x) + (n_y c_y)) + (n_z c_z) > 0: it faces the camera (regnet_depth_normals_f32's rule).
 *   colour      rgb NULL: none.  Else the values of C_r, C_g, C_b at p when that sample is known, else 0.
 * Outputs, DEVICE memory, written whole: xyz, normals (height width, 3) float32, row v width + u, IN THE VIRTUAL CAMERA's frame
 * (regnet_icp_step_projective_f32's target layout): the quiet NaN 0x7FC00000 in xyz without a hit and in normals without a normal;
 * rgb (height width, 3) float32 or NULL: 0 without a hit; status (height width) uint8: 0 no surface, 1 back face, 2 hit, 3 hit
 * without normal; counts (4) int32: the histogram of status, cleared by a one-workgroup kernel, then one integer atomic per
 * workgroup and code.  Two launches; 16 x 16 pixels per 256-thread workgroup, an 8 x 8 tile per wave.
 *   clip        != 0: a ray visits only the samples between which a slab test (float64, the box of voxel centres grown by a voxel
 *               and by 2^-18 of every magnitude entering p, the range by one sample either way) says it can be inside; the rest
 *               are unknown by the sample rule, so clip changes the time and no bit of the result.  0: every sample is visited.
 *               The slack is an ARGUED bound (at most 8 roundings of 2^-24 enter p and g, the slack allows 64), not a proven
 *               one; it is held by the bit-for-bit comparison with a restatement that clips nothing, and clip = 0 is the way out.
 * No host read, no synchronisation, no allocation, no cooperative launch, no floating-point atomic: capturable.  Errors, all before
 * any launch: a dim, width, height, min_weight or n_steps < 1 -> REGNET_ERR_SHAPE; N > 2^28, a dim > 2^24, width height > 2^21,
 * n_steps > 4096, voxel, near or step not finite or not positive (in float32 too) -> REGNET_ERR_UNSUPPORTED; a NULL pointer for a
 * required array (all but rgb) -> REGNET_ERR_NULL.                                                                            */
int regnet_tsdf_raycast_f32(const void* volume, int64_t nx, int64_t ny, int64_t nz, const float* origin3, double voxel,
                            int64_t min_weight, const float* intrinsics4, const float* pose12, double near, double step,
                            int64_t n_steps, int64_t width, int64_t height, int clip, float* xyz, float* normals, float* rgb,
                            uint8_t* status, int32_t* counts, void* stream);

/* ---- pose refinement (csrc/icp.hip): point-to-plane ICP of a source cloud onto a target cloud with normals, on the device ----
 * What corrects a camera pose before the merge above.  Correspondences are decided on canonical fp32 arithmetic (individually
 * rounded binary32 operations in the written order, -ffp-contract=off); residuals, normal equations, solve and pose update are
 * float64 with one rounding per operation.  Every sum is formed in a fixed order and no floating-point atomic is used: two runs
 * agree bit for bit.
 *   target      target_xyz (N_t,3) float32 contiguous, every coordinate finite (the caller compacts); target_normals (N_t,3)
 *               float32 contiguous, row j the normal of target row j.
 *   source      source_xyz (N_s,3) float32 contiguous.  The step visits every `stride`-th row: visited row k is source row
 *               k * stride, k = 0 .. rows - 1, rows = ceil(N_s / stride).  A row with a non-finite coordinate is skipped.
 *               (A stride above 2^21 is taken as 2^21: one visited row.  On the row-by-row cloud of a depth image a stride that
 *               divides the image width visits whole pixel columns only: the caller's concern.)
 *   state       regnet_icp_state_bytes() = 1152 bytes, DEVICE, 16-byte aligned, written by the caller before the first step:
 *                 offset   0  pose[12] float64: rows 0..2 of the row-major 4x4 source-to-target transform
 *                 offset  96  int32 iteration (steps run, 0 at the start), status (0 at the start), max_iter (1..64), 0
 *                 offset 112  float64 rot_eps [rad], trans_eps [m]
 *                 offset 128  history[64][2] float64: per step run (pairs, rms = sqrt(sum r r / pairs), 0 without a pair), the
 *                             residuals being those BEFORE the step's update
 *               status: 0 RUNNING, 1 CONVERGED, 2 MAX_ITER, 3 TOO_FEW, 4 DEGENERATE.  When the status is not RUNNING both
 *               launches of a step return at once and write nothing -- not the state, not idx_out, not sums_out -- so a caller
 *               enqueues a fixed number of steps and reads the state once.
 *   pose        each entry of state.pose rounded once to float32 (to nearest even), then p = ((r0 x + r1 y) + r2 z) + r3 per
 *               coordinate: regnet_fuse_accumulate_f32's expression.  A p with a non-finite coordinate has no match.
 *   match       the target row smallest by (d2, row), d2 = ((dx dx) + (dy dy)) + (dz dz) with dx = p_x - q_x, accepted when
 *               d2 <= float32(max_dist * max_dist) (the product in float64, rounded once).  The uniform grid (csrc/grid.h,
 *               requested cell edge max_dist, coarsened by itself to stay within 65536 cells) only decides which pairs are
 *               evaluated: the cells overlapping the ball of max_dist around p, widened by the header's rounding margin, so the
 *               result does not depend on the cell edge.
 *   idx_out     (rows) int32 or NULL: the accepted target row of visited row k, -1 when rejected, -2 when the row was skipped.
 *   terms       per accepted pair, float64 from the float32 values: r = ((n_x (p_x - q_x)) + (n_y (p_y - q_y))) + (n_z (p_z - q_z)),
 *               a = (p x n, n) = (p_y n_z - p_z n_y, p_z n_x - p_x n_z, p_x n_y - p_y n_x, n_x, n_y, n_z).
 *   sums_out    (29) float64 or NULL: a_u a_v for u <= v in row-major order (21), a_u r (6), r r, the pair count.  Summed over a
 *               wave by a butterfly of lane exchanges (distance 32, 16, .. 1), the four waves of a workgroup in order, one slot
 *               per workgroup of 256 visited rows; then the slots in 8 contiguous runs, ascending inside a run, the runs in order.
 *   solve       the history row and the iteration counter are written first.  pairs < min_pairs -> TOO_FEW, pose unchanged.  Else
 *               H x = -g, H the 6x6 of a a^T and g the 6 of a r, by a Cholesky factorisation H = L L^T row by row: a pivot
 *               L_uu^2 = H_uu - sum_w L_uw^2 that is not above 1e-12 * max_u H_uu (a NaN one included) -> DEGENERATE, pose
 *               unchanged (one flat table-top leaves three of the six motions free).
 *   update      w = x[0:3], t = x[3:6], theta = |w|; R = I + A K + B (w w^T - theta^2 I), K the cross-product matrix of w,
 *               A = sin(theta) / theta, B = (1 - cos(theta)) / theta^2, and below theta = 1e-6 A = 1 - theta^2 / 6,
 *               B = 1 / 2 - theta^2 / 24.  pose <- [R | t] . pose, each entry (R_u0 T_0w + R_u1 T_1w) + R_u2 T_2w, + t_u in the
 *               last column.  Then CONVERGED when theta < rot_eps and |t| < trans_eps, else MAX_ITER when iteration == max_iter.
 * workspace: regnet_icp_workspace_bytes(N_t, N_s) bytes, 16-byte aligned: the grid slab of the target and 256 bytes per workgroup
 * of 256 source rows; -1 for a count outside [0, 2^21].  regnet_icp_prepare_f32 builds the grid (four short launches) and is
 * called once per target; regnet_icp_step_f32 is one iteration, two launches (A: a lane per visited row over all CUs; B: one
 * workgroup), with the N_t and max_dist of the prepare.  No host read, no synchronisation, no allocation.  N_s == 0: launch B alone
 * (no pair).  N_t == 0: no row has a match.  Errors, all before any launch: a negative count, stride < 1 or min_pairs < 0 ->
 * REGNET_ERR_SHAPE; a count above 2^21, max_dist not finite, <= 0 or outside float32's range -> REGNET_ERR_UNSUPPORTED; a NULL
 * pointer for a required array -> REGNET_ERR_NULL.                                                                            */
int64_t regnet_icp_state_bytes(void);
int64_t regnet_icp_workspace_bytes(int64_t N_target, int64_t N_source);
int regnet_icp_prepare_f32(const float* target_xyz, int64_t N_target, double max_dist, void* workspace, void* stream);
int regnet_icp_step_f32(const float* source_xyz, int64_t N_source, int64_t stride, const float* target_normals, int64_t N_target,
                        void* state, double max_dist, int32_t* idx_out, double* sums_out, int64_t min_pairs, void* workspace,
                        void* stream);

/* Projective association: regnet_icp_step_projective_f32 is the same step for a target that is the ORGANISED cloud of a depth
 * image in the TARGET CAMERA's frame -- a lookup in the target's image instead of a search over a grid, and no prepare call.
 * State block, status codes, terms, sums, solve and update are those above; only launch A differs (icp_project_kernel).
 *   target      target_xyz, target_normals (H W, 3) float32 DEVICE, row v W + u for pixel (u, v); NaN marks a removed pixel or a
 *               pixel without a normal (regnet_depth_normals_f32).  state.pose takes the source into the target CAMERA's frame.
 *   intrinsics  (4) float64 HOST memory: fx, fy, cx, cy of the target's camera, each rounded once to float32.
 *   row         visited as above; a row with a non-finite coordinate is skipped (-2).  p as above; a p with a non-finite
 *               coordinate, or whose p_z is not > 0, has no match (-1).
 *   pixel       regnet_depth_to_cloud_*'s projection: uf = (p_x / p_z) * fx + cx with the correctly rounded division,
 *               fu = floorf(uf + 0.5f), inside when fu >= 0 && fu < W in float (a NaN fails); likewise fv.  Outside: -1.
 *   candidates  the pixels (u + a, v + b), |a|, |b| <= window (0..2), inside the image, whose three coordinates and three normal
 *               components are all finite.
 *   normal gate on unless min_cos < -1: source_normals (N_s, 3) float32 DEVICE, row i the normal of source row i in the SOURCE's
 *               frame; m = R s with the float32 rotation of p, m_x = ((r0 s_x) + (r1 s_y)) + (r2 s_z) and likewise m_y, m_z; a
 *               candidate must satisfy ((m_x n_x) + (m_y n_y)) + (m_z n_z) >= float32(min_cos).  A source row with a non-finite
 *               normal has no candidate (-1).  source_normals may be NULL exactly when the gate is off (or N_s == 0).
 *   match       the candidate smallest by (d2, row), row = v W + u, accepted when d2 <= float32(max_dist * max_dist).
 *   idx_out     (rows) int32 or NULL: the accepted target row, -1, or -2.
 * workspace: regnet_icp_projective_workspace_bytes(N_s) bytes, 16-byte aligned: 256 bytes per workgroup of 256 visited rows (at
 * least one); -1 for a count outside [0, 2^21].  Two launches, no host read, no synchronisation, no allocation, no floating-point
 * atomic.  N_s == 0: launch B alone.  Errors, all before any launch: as regnet_icp_step_f32 with W < 1 or H < 1 for the target's
 * count, and window outside 0..2 -> REGNET_ERR_SHAPE; W H > 2^21, fx or fy not finite or not positive (in float32 too), min_cos
 * > 1 or NaN -> REGNET_ERR_UNSUPPORTED.                                                                                      */
int64_t regnet_icp_projective_workspace_bytes(int64_t N_source);
int regnet_icp_step_projective_f32(const float* source_xyz, int64_t N_source, int64_t stride, const float* source_normals,
                                   const float* target_xyz, const float* target_normals, int64_t W, int64_t H,
                                   const double* intrinsics, int64_t window, void* state, double max_dist, double min_cos,
                                   int32_t* idx_out, double* sums_out, int64_t min_pairs, void* workspace, void* stream);

/* regnet_icp_state_continue: the hand-over of ONE state block between the levels of a coarse-to-fine registration.  One thread,
 * one launch, ordered by the stream after the steps enqueued before it.
 *   mark        (2) int32 DEVICE or NULL: (iteration, status) as found, stored first.
 *   rule        status CONVERGED or MAX_ITER: the pose and the history stay, status = RUNNING,
 *               max_iter = min(64, iteration + budget) -- the steps enqueued next run, at most `budget` of them.  Any other
 *               status leaves the block untouched: RUNNING is left alone, TOO_FEW and DEGENERATE stay final, so the steps of the
 *               later levels return at once.
 * Errors, before the launch: budget outside 1..64 -> REGNET_ERR_SHAPE; state NULL -> REGNET_ERR_NULL.                       */
int regnet_icp_state_continue(void* state, int64_t budget, int32_t* mark, void* stream);

/* ---- approach analysis (csrc/approach.hip): clearance on the way in, closing extent and contact check per grasp, on the device ----
 * What turns a collision-free grasp into a motion.  regnet_grasp_collision_counts_f32 above tests the hand at the final pose
 * only; this scan also sweeps the hand back along -approach, measures the object between the fingers and judges the two contact
 * bands on the cloud's normals.  points (N,3) float32, element strides (pn, pc) for (point, coordinate); normals (N,3) float32,
 * element strides (nn, nc), row j the normal of point j, or NULL; T (B,4,4) row-major global->local, contiguous;
 * x_hi_per_grasp (B) overrides x_hi when not NULL.  One workgroup per grasp, two passes over the cloud.  Canonical fp32
 * arithmetic: individually rounded binary32 operations in the written order (-ffp-contract=off), the local point being
 *   x = ((t00 px + t01 py) + t02 pz) + t03,  y and z likewise from rows 1 and 2 of T[b]
 * (regnet_grasp_collision_counts_f32's expression).  Every comparison is strict, as in the reference's box tests; a point with a
 * NaN coordinate is in nothing.  With xh the grasp's x_hi, ht = half_thickness, hw = half_width, hs = half_space, S = standoff:
 *   section   z < ht && z > -ht && y < hw && y > -hw
 *   inner     section && y < hs && y > -hs
 *   region    inner && x > x_lo && x < xh: the reference's closing region, counts[:,3] of regnet_grasp_collision_counts_f32
 *   pass 1    n_region; y_min, y_max, x_min over the region; n_hand = behind the hand + inside a finger exactly as
 *             regnet_grasp_collision_counts_f32 counts them (its columns 1 + 2: a hand that collides at the final pose shows).
 *             The sweep: a point is a BLOCKER when section && x < front && x > x_lo - S, front = back_x for inner points and xh
 *             for the rest of the section (the finger lanes, |y| == hs included); x_lo - S is one float32 subtraction.  Its
 *             retreat is s = fmaxf(x_lo - x, 0.0f).  n_block = the number of blockers; clearance = fminf(S, min s) over them, S
 *             without one: the longest straight retreat along -approach from the final pose that touches nothing, capped at S.
 *   pass 2    skipped when normals == NULL (its four counts are then 0).  band = min((y_max - y_min) / 3.0f, contact_depth);
 *             left band = the region points with y > y_max - band, right band = those with y < y_min + band
 *             (regnet_grasp_antipodal_stats_f32's rule).  Per band, n = its size and ok = the number of its points with
 *             fabsf((t10 nx + t11 ny) + t12 nz) >= cos_friction; a NaN normal fails.
 *   counts    (B,8) int32: { n_region, n_block, n_hand, n_left, ok_left, n_right, ok_right, 0 }.
 *   values    (B,4) float32: { y_min, y_max, clearance, x_min }, each + 0.0f before the store (-0.0 never leaves the kernel);
 *             with n_region == 0: +inf, -inf, clearance, +inf.
 * Only integer sums and float min / max are reduced: no floating-point sum and no atomic, so the result does not depend on the
 * order of the reduction and two runs agree bit for bit.  One launch; no host read, no synchronisation, no allocation: capturable.
 * B == 0: success without a launch.  N == 0: launches and writes the empty results.  Errors, all before any launch: a negative
 * count -> REGNET_ERR_SHAPE; a count >= 2^31, or a standoff that is negative or not finite -> REGNET_ERR_UNSUPPORTED; a NULL T,
 * counts or values, or NULL points with N > 0 -> REGNET_ERR_NULL.                                                             */
int regnet_grasp_approach_f32(const float* points, int64_t pn, int64_t pc, const float* normals, int64_t nn, int64_t nc,
                              int64_t N, const float* T, int64_t B, float x_lo, float x_hi, const float* x_hi_per_grasp,
                              float half_thickness, float half_width, float half_space, float back_x, float standoff,
                              float contact_depth, float cos_friction, int32_t* counts, float* values, void* stream);

/* ---- approach analysis against the TSDF volume (csrc/approach_volume.hip): occupied and unseen space per grasp, on the device ----
 * regnet_grasp_approach_f32 above holds the swept hand against the points a camera saw; to it the occluded back of an object and
 * the space no view reached are free.  This scan holds the same hand against the volume of the TSDF section above, which knows
 * three states per voxel: seen solid, seen free, never observed.  It scans no points but a LATTICE of samples of the swept hand
 * in the grasp's local frame, so its cost follows the hand's volume.  The volume is only read (D and W).  One workgroup of 256
 * threads per grasp.  Canonical fp32 arithmetic: individually rounded binary32 operations in the written order
 * (-ffp-contract=off), divisions correctly rounded (__fdiv_rn), every comparison strict unless written otherwise.
 *   volume, dims, origin3 (3 float32, HOST), voxel, min_weight   as for regnet_tsdf_emit_f32; every dim <= 2^24.
 *               voxel_f = float32(voxel).  d_solid = float32(margin / trunc), the division in float64, rounded once.
 *   box         x_lo, x_hi, x_hi_per_grasp (B, DEVICE, or NULL), half_thickness ht, half_width hw, half_space hs, back_x,
 *               standoff S: regnet_grasp_approach_f32's, xh being the grasp's x_hi.
 *   lattice     shared by all grasps of the call.  h = float32(step).  xs = x_lo - S, one float32 subtraction (the sweep's far
 *               end of regnet_grasp_approach_f32).  n_x = max(1, ceil((x_extent - xs) / h)), n_y = max(1, ceil((hw + hw) / h)),
 *               n_z = max(1, ceil((ht + ht) / h)), evaluated on the host in float64 from the float32 values.  x_extent is x_hi,
 *               or with x_hi_per_grasp the caller's bound on them (samples beyond a grasp's own xh drop out by the strict
 *               tests below; a grasp whose xh lies beyond x_extent is analysed up to x_extent only).  Sample (i, j, k), cell
 *               centred and never accumulated:
 *                 x_i = xs + (((float)i + 0.5f) * h),  y_j = (((float)j + 0.5f) * h) - hw,  z_k = (((float)k + 0.5f) * h) - ht.
 *   sets        regnet_grasp_approach_f32's predicates (one definition, csrc/hand_box.h), on the sample's local (x, y, z):
 *                 section = z < ht && z > -ht && y < hw && y > -hw;  inner = section && y < hs && y > -hs;
 *                 close = x > x_lo && x < xh;  region = inner && close;
 *                 back = section && close && x < back_x;  finger = section && close && (y > hs || y < -hs);
 *                 HAND membership = (int)back + (int)finger (a sample that is both counts twice, as there);
 *                 BLOCKER = section && x < front && x > xs, front = back_x for inner samples and xh for the rest of the section;
 *                 its retreat s = fmaxf(x_lo - x, 0.0f).
 *               A sample in none of region, hand, blocker is not looked up.
 *   lookup      L (B,12) float32 DEVICE: per grasp rows 0..2 of the row-major 4x4 LOCAL-TO-VOLUME transform.
 *                 wx = (((l00 x) + (l01 y)) + (l02 z)) + l03, wy and wz likewise from rows 1 and 2.
 *               Per axis c = floorf(__fdiv_rn(w - o, voxel_f)): voxel i covers [o + i voxel, o + (i + 1) voxel), its centre being
 *               the TSDF section's.  INSIDE iff c >= 0 && c < (float)n on all three axes, compared in float (a NaN fails).  The
 *               voxel is the NEAREST one: nothing is interpolated.
 *   class       OUTSIDE: not inside.  UNKNOWN: W < min_weight, or D is a NaN.  SOLID: D < d_solid.  FREE: everything else
 *               (D == 1, the value of a voxel a view looked through, included).  UNSEEN = OUTSIDE or UNKNOWN.  One W is loaded
 *               per looked-up sample and D only when W >= min_weight.
 *   counts      (B,8) int32: { region SOLID, region UNSEEN, hand SOLID, hand UNSEEN, blockers SOLID, blockers UNSEEN, M, M_out }:
 *               hand counts are sums of the hand membership; M = the sum over the looked-up samples of (hand membership +
 *               (int)blocker), the denominator that goes with columns 3 + 5, and M_out the part of M on OUTSIDE samples.
 *   values      (B,4) float32: { y_min, y_max over the region's SOLID samples, clearance_seen = fminf(S, min s over the SOLID
 *               blockers), clearance_safe = fminf(S, min s over the SOLID or UNSEEN blockers) }, each + 0.0f before the store;
 *               an empty set gives +inf, -inf, S, S.  Both clearances and y_min / y_max are sample coordinates: quantised to
 *               the lattice.
 * Only integer sums and float min / max are reduced (a wave butterfly, then the four waves through LDS): no atomic and no
 * floating-point sum, so two runs agree bit for bit.  A wave takes 8 x 8 tiles of the lattice's x-y plane and walks the z layers.
 * One launch; no host read, no synchronisation, no allocation: capturable.  A row of L with a non-finite entry launches and
 * reports every looked-up sample OUTSIDE (M_out == M).  Errors, all before any launch: B < 0, a dim < 1 or min_weight < 1 ->
 * REGNET_ERR_SHAPE; a dim > 2^24, nx ny nz > 2^28, B or min_weight >= 2^31, step, voxel or trunc not finite or not positive (in
 * float32 too), a standoff that is negative or not finite, margin / trunc not finite in float32, a lattice count that is not
 * finite or n_x n_y n_z > 2^22 -> REGNET_ERR_UNSUPPORTED; then B == 0: success without a launch; then a NULL volume, origin3, L,
 * counts or values -> REGNET_ERR_NULL.                                                                                       */
int regnet_grasp_approach_volume_f32(const void* volume, int64_t nx, int64_t ny, int64_t nz, const float* origin3, double voxel,
                                     double trunc, int64_t min_weight, double margin, const float* L, int64_t B, float x_lo,
                                     float x_hi, const float* x_hi_per_grasp, float half_thickness, float half_width,
                                     float half_space, float back_x, float standoff, double step, float x_extent,
                                     int32_t* counts, float* values, void* stream);

/* ---- distance field of the TSDF volume (csrc/edt.hip): how much room there is, per voxel, per point and per grasp ----------------
 * The approach analysis above says whether a sample of the hand is SOLID, UNSEEN or FREE.  The distance field says how far every
 * voxel is from the nearest obstacle voxel: the exact Euclidean distance transform of the volume's lattice.  Squared distances in
 * voxel units are integers, so everything below is integer work and is compared with tests/edt_reference.py with no tolerance;
 * two runs give the same bytes.
 *
 * Field.  regnet_tsdf_edt(volume, dims, trunc, min_weight, margin, mode, outside, dist2, nearest, stream)
 *   volume      the five planes of the section above; only D and W are read.
 *   class       a voxel is classed as regnet_grasp_approach_volume_f32 classes a sample's voxel: UNKNOWN when W < min_weight or D
 *               is a NaN; SOLID when D < d_solid = float32(margin / trunc) (the division in float64, rounded once); FREE
 *               otherwise.  The OBSTACLES are the SOLID voxels (mode 0) or the SOLID and UNKNOWN voxels (mode 1).
 *   dist2       (N) int32 DEVICE, word l = (iz ny + iy) nx + ix: the minimum over the obstacle voxels q of |v - q|^2 in voxel
 *               units (between voxel centres), 0 on an obstacle, REGNET_EDT_NONE = 2^30 everywhere when there is no obstacle.
 *   nearest     (N) int32 DEVICE or NULL: the linear index of an obstacle voxel at that distance; of all of them the one with the
 *               SMALLEST LINEAR INDEX, i.e. the lexicographic minimum in (iz, iy, ix); -1 where dist2 == REGNET_EDT_NONE.
 *   outside     1: everything beyond the six faces is an obstacle too (the approach analysis' OUTSIDE is UNSEEN).  The slab beyond
 *               a face is nearest along that axis, so with m = min over the axes of min(i + 1, n - i): dist2 = min(dist2, m^2),
 *               and nearest = -1 where m^2 is STRICTLY below the distance to every interior obstacle (an interior obstacle wins
 *               a tie).
 *   limits      every dim in 1..1024 and N <= 2^28, so dist2 <= 3 * 1023^2 < 2^22 wherever it is not REGNET_EDT_NONE.
 * Three launches -- a line pass along x, y and z -- that run in place in dist2 / nearest, the only workspace; no host read, no
 * synchronisation, no allocation: capturable.  No atomic, no sort.  Errors, all before any launch: a dim or min_weight < 1, mode or
 * outside not 0 / 1 -> REGNET_ERR_SHAPE; a dim > 1024, N > 2^28, min_weight >= 2^31, trunc, margin or margin / trunc not finite in
 * float32 -> REGNET_ERR_UNSUPPORTED; a NULL volume or dist2 -> REGNET_ERR_NULL.
 * regnet_tsdf_edt_pass is ONE of the three launches, pass = 0, 1, 2 for x, y, z (a measurement; pass outside 0..2 ->
 * REGNET_ERR_SHAPE): the three in order are regnet_tsdf_edt.  regnet_edt_tile(n, with_nearest): the lines of consecutive ix a
 * workgroup of the y / z pass stages for an axis of n voxels -- 64, 32, 16 or 8, the largest whose tile stays within 64 KiB --,
 * REGNET_ERR_UNSUPPORTED for n outside 1..1024; a host function.
 *
 * Query.  regnet_edt_query_f32: one lane per point, one launch.
 *   points      (M,3) float32 DEVICE, element (m, k) at points[m stride_row + k stride_col].  T12: 12 float32 on the HOST, rows
 *               0..2 of the row-major to-volume 4x4:  wx = (((t00 x) + (t01 y)) + (t02 z)) + t03, wy and wz likewise.
 *   lookup      origin3, voxel as above, voxel_f = float32(voxel); per axis c = floorf(__fdiv_rn(w - o, voxel_f)), INSIDE iff
 *               c >= 0 && c < (float)n on all three axes, compared in float (a NaN fails): the lookup of the section above.
 *   distance    (M) float32: sqrtf((float)d2) * voxel_f, + 0.0f before the store -- the conversion is exact, the root correctly
 *               rounded, the product one operation --; +inf for REGNET_EDT_NONE; the quiet NaN 0x7fc00000 for a point that is
 *               not INSIDE.
 *   nearest_xyz (M,3) float32 contiguous or NULL: the centre o_k + (((float)i_k + 0.5f) * voxel_f) of the nearest obstacle voxel,
 *               in the volume's frame; NaN where there is none (nearest NULL or -1, or the point not INSIDE).
 * M == 0: success without a launch.  Errors: M < 0 or a dim < 1 -> REGNET_ERR_SHAPE; a dim > 1024, N > 2^28, M >= 2^31, voxel not
 * finite or not positive (in float32 too) -> REGNET_ERR_UNSUPPORTED; then M == 0; then a NULL dist2, origin3, points, T12 or
 * distance -> REGNET_ERR_NULL.
 * regnet_edt_metres_f32(dist2, n, voxel, out): out[l] = the query's distance of word l, for n words (the whole field, or any
 * array of squared distances); n == 0: success; n < 0 -> REGNET_ERR_SHAPE, n > 2^28 or a bad voxel -> REGNET_ERR_UNSUPPORTED.
 *
 * Margin.  regnet_grasp_margin_volume_f32: the swept hand of regnet_grasp_approach_volume_f32 -- the same lattice, the same
 * L (B,12), the same sets (csrc/hand_box.h) and the same lookup (one definition, csrc/hand_lattice.h) -- read against dist2.
 *   samples     a HAND sample is one with back || finger at the final pose, a SWEPT sample one that is a hand sample or a
 *               BLOCKER.  Only swept samples are looked up (the region between the fingers is not part of the hand).
 *   margins     (B,2) int32: { the minimum dist2 over the hand samples, the minimum over the swept samples }, REGNET_EDT_NONE
 *               where the set is empty.  An OUTSIDE sample contributes 0 when outside = 1 (it lies in an obstacle of a field
 *               built with outside = 1) and nothing otherwise.
 *   counts      (B,4) int32: { hand samples, hand samples OUTSIDE, swept samples, swept samples OUTSIDE } -- samples, not
 *               memberships: a sample that is back and finger counts once.
 * One workgroup of 256 threads per grasp, the tile walk of the approach analysis; integer minima and sums only (a wave butterfly,
 * then the four waves through LDS), no atomic.  One launch, capturable.  A row of L with a non-finite entry reports every swept
 * sample OUTSIDE.  Errors, all before the launch: B < 0, a dim < 1, outside not 0 / 1 -> REGNET_ERR_SHAPE; a dim > 1024, N > 2^28,
 * B >= 2^31, step or voxel not finite or not positive (in float32 too), a standoff that is negative or not finite, a lattice count
 * that is not finite or n_x n_y n_z > 2^22 -> REGNET_ERR_UNSUPPORTED; then B == 0: success without a launch; then a NULL dist2,
 * origin3, L, margins or counts -> REGNET_ERR_NULL.
 *
 * Signed, capped field.  regnet_tsdf_sdf(volume, dims, trunc, min_weight, margin, mode, outside, sign, cap, field, nearest, work,
 * stream): volume, the classification, mode, outside, margin, min_weight and the limits are regnet_tsdf_edt's.
 *   sign = 0    field is dist2 as above.
 *   sign = 1    field (N) int32 holds SIGNED squared voxel distances: a non-obstacle voxel v gets +min |v - q|^2 over the obstacle
 *               voxels q (>= 1), an obstacle voxel gets -min |v - p|^2 over the NON-obstacle voxels p of the lattice (<= -1); 0
 *               never occurs.  No obstacle at all: every word +REGNET_EDT_NONE; no free voxel: every word -REGNET_EDT_NONE.
 *               outside = 1 adds the slabs beyond the faces to the obstacles of the positive side (min(d2, m^2) as above); the
 *               outside is never free space and does not enter the negative side.
 *   cap         int64, in voxels: 0 none, else 1..1023.  Values saturate: min(d2, cap^2) on the positive side, max(-d2, -cap^2)
 *               on the negative one, +-NONE becomes +-cap^2.  The search of every line pass stops at d > cap, at most 2 cap + 1
 *               words per voxel and pass wherever the obstacles are; the result is exact all the same (DESIGN.md par. 5).  A
 *               true distance of exactly cap is a real value.
 *   nearest     (N) int32 or NULL: for a non-obstacle voxel the nearest obstacle voxel; for an obstacle voxel with sign = 1 the
 *               nearest non-obstacle voxel, the way out; of several the smallest linear index on both sides.  -1 where the value
 *               is +-NONE, where it is saturated STRICTLY beyond the cap (a distance of exactly cap keeps its nearest), or where a
 *               face slab is strictly nearer.
 *   work        DEVICE scratch of regnet_tsdf_sdf_workspace_bytes(nx, ny, nz, sign, with_nearest) bytes (a host function: 0 with
 *               sign = 0 or bad dims, else 4 N, 8 N with nearest), 4-byte aligned: the planes of the second transform.
 * sign = 0: the three launches above; sign = 1: six -- the three passes with the obstacles as seeds into field / nearest, then
 * the three over the COMPLEMENT (the non-obstacle voxels as seeds) in work, whose z pass writes minus its result into the words
 * of field that are 0.  No allocation, host read or synchronisation, no atomic: capturable, and two runs give the same bytes.
 * With sign = 0 and cap = 0 the output equals regnet_tsdf_edt's byte for byte.  Errors, all before any launch and in
 * regnet_tsdf_edt's order: sign not 0 / 1 or cap < 0 with the REGNET_ERR_SHAPE rules; cap > 1023 with the REGNET_ERR_UNSUPPORTED
 * rules (after the dims); a NULL work where the size is non-zero with the REGNET_ERR_NULL rules.
 *
 * Signed metres.  regnet_edt_metres_signed_f32(field, n, voxel, out): for a signed word s, a = sqrtf((float)|s|) and
 * out = copysignf((a - 0.5f) * voxel_f, (float)s), every operation rounded on its own, + 0.0f before the store; +-inf for +-NONE.
 * The half voxel makes it the distance to the boundary FACE between the classes, not to a voxel centre: across an axis-aligned
 * wall consecutive centres read ..., -1.5, -0.5, +0.5, +1.5, ... voxels, the true signed distance and a linear function.  n and
 * voxel as in regnet_edt_metres_f32, which is unchanged.
 *
 * Signed query.  regnet_edt_query_signed_f32: one lane per point, one launch; points, T12, the transform and the INSIDE rule are
 * regnet_edt_query_f32's; a point that is not INSIDE gets the quiet NaN 0x7fc00000 in every output.
 *   interpolate = 0   distance (M) float32 = the signed metres of the point's nearest voxel; gradient, if given, NaN.
 *   interpolate = 1   trilinear between the eight voxel centres around the point.  Per axis u = __fdiv_rn(w - o, voxel_f) - 0.5f,
 *               i0 = floorf(u), t = u - i0; the corner indices i0 and i0 + 1 are each clamped to [0, n - 1] (in the outer
 *               half-voxel rim the interpolation degenerates to the nearest layer along that axis).  The corner values are the
 *               signed metres above; lerp(a, b, t) = a + (t * (b - a)), applied along x, then y, then z.
 *   gradient    (M,3) float32 contiguous or NULL: the analytic derivative of that interpolant in the VOLUME's frame.  For an
 *               axis, the four differences b - a of the corner values along it, each __fdiv_rn(b - a, voxel_f), lerped over the
 *               other two axes, x before y before z.  Dimensionless, length 1 across a flat wall.
 *   nearest_xyz as in regnet_edt_query_f32, for the point's nearest voxel (the way out for a point in an obstacle voxel).
 * Non-finite results are what IEEE arithmetic gives (infinite corners of an uncapped field: inf - inf); any NaN is stored as
 * 0x7fc00000.  Use a cap with interpolation.  Errors: regnet_edt_query_f32's; interpolate not 0 / 1 -> REGNET_ERR_SHAPE.
 *
 * Signed margin.  regnet_grasp_margin_volume_signed_f32: regnet_grasp_margin_volume_f32 (one kernel, a template parameter)
 * reading a signed plane.  margins (B,2) int32 are the signed minima over the hand and over the swept samples: a negative value
 * is minus the squared depth in voxels of the deepest sample.  An OUTSIDE sample under outside = 1 contributes -1 (an obstacle
 * of unknown depth; 0 is not a value of a signed field).  counts (B,6) int32: the four above, then the hand samples with a
 * negative value, then the swept samples with one (OUTSIDE samples under outside = 1 included).  Errors, launch and reductions
 * as in the unsigned entry, which is unchanged.
 *
 * Retreat fan (csrc/retreat.hip).  regnet_grasp_retreat_fan_f32 / regnet_grasp_retreat_fan_signed_f32 (one kernel, a template
 * parameter): the rigid hand at its FINAL pose moved along R candidate directions in K steps and read against the field at every
 * step.  field, dims, origin3 (HOST), voxel, outside, L (B,12), the box arguments, step, x_extent and the limits on the dims are
 * the margin entries'; the lookup is theirs (csrc/hand_lattice.h).  Canonical fp32 arithmetic as everywhere in this family.
 *   lattice     the margin entries' with standoff = 0: xs = x_lo.  Only HAND samples are used -- back || finger, a sample that
 *               is both counted once; the region between the fingers is not part of the hand.  Membership is decided once per
 *               sample, at the final pose.
 *   dirs        DEVICE float32, in the grasp's LOCAL frame: row (b, r) at dirs + b dirs_grasp_stride + 3 r; a stride of 0 is one
 *               table shared by all grasps.  R in 1..16.  Not normalised: the vector is used as given.
 *   steps       k = 0 .. K, K in 1..64.  ds_f = float32(ds), t_k = (float)k * ds_f; the sample (x, y, z) at step k is
 *               (x + (t_k * d_x), y + (t_k * d_y), z + (t_k * d_z)) and then goes through L as the margin entries' samples do.
 *               Step 0 is the final pose for every finite direction.
 *   value       the field word of the sample's voxel.  An OUTSIDE sample contributes 0 (signed: -1) under outside = 1 and
 *               nothing under outside = 0.  A non-finite position (a NaN row of L, a NaN direction -- at step 0 too, 0 * NaN
 *               being a NaN) is OUTSIDE.
 *   profile     (B, R, K + 1) int32 or NULL: the minimum value over the hand samples at each step, REGNET_EDT_NONE for an empty
 *               set.
 *   result      (B, R, 4) int32: { free_steps = the largest n in 0..K with profile[k] >= thresh for all 1 <= k <= n (step 0 is
 *               not judged: a hand that collides at the final pose is the margin's business); the minimum of profile over steps
 *               1..free_steps, REGNET_EDT_NONE when free_steps is 0; the minimum over steps 1..K; the number of OUTSIDE lookups
 *               over steps 1..K, whatever `outside` says }.
 * One workgroup of 256 threads per (grasp, direction), the tile walk of the approach analysis.  The per-step minima are LDS
 * words lowered by LDS integer minima (a minimum has no order), the OUTSIDE count an integer sum (a wave butterfly, then the four
 * waves through LDS): no floating-point sum, no global atomic, no host read, no allocation; capturable; two runs give the same
 * bytes.  Errors, all before the launch: B < 0, a dim < 1, outside not 0 / 1, R or K < 1, a negative dirs_grasp_stride ->
 * REGNET_ERR_SHAPE; a dim > 1024, N > 2^28, B >= 2^31, step or voxel not finite or not positive (in float32 too), R > 16, K > 64,
 * B R (K + 1) > 2^28, ds negative or not finite (in float32 too; ds == 0 is allowed, every step then equals step 0), a lattice
 * count that is not finite or n_x n_y n_z > 2^22 -> REGNET_ERR_UNSUPPORTED; then B == 0: success without a launch; then a NULL
 * field, origin3, L, dirs or result -> REGNET_ERR_NULL.
 *
 * Pick.  regnet_grasp_retreat_pick(result, B, R, best, stream): one lane per grasp.  best (B,4) int32 = { r*, free_steps of r*,
 * its free-prefix minimum, 0 }: r* is the direction with the most free steps; among equals the larger free-prefix minimum wins;
 * among equals of that the smallest r -- the caller lists the directions in order of preference.  Errors: B < 0 or R < 1 ->
 * REGNET_ERR_SHAPE; R > 16 or B >= 2^31 -> REGNET_ERR_UNSUPPORTED; then B == 0: success; then a NULL result or best ->
 * REGNET_ERR_NULL.                                                                                                            */
#define REGNET_EDT_NONE (1 << 30)
int regnet_grasp_retreat_fan_f32(const int32_t* field, int64_t nx, int64_t ny, int64_t nz, const float* origin3, double voxel,
                                 int outside, const float* L, int64_t B, float x_lo, float x_hi, const float* x_hi_per_grasp,
                                 float half_thickness, float half_width, float half_space, float back_x, double step,
                                 float x_extent, const float* dirs, int64_t dirs_grasp_stride, int64_t R, int64_t K, double ds,
                                 int thresh, int32_t* profile, int32_t* result, void* stream);
int regnet_grasp_retreat_fan_signed_f32(const int32_t* field, int64_t nx, int64_t ny, int64_t nz, const float* origin3,
                                        double voxel, int outside, const float* L, int64_t B, float x_lo, float x_hi,
                                        const float* x_hi_per_grasp, float half_thickness, float half_width, float half_space,
                                        float back_x, double step, float x_extent, const float* dirs, int64_t dirs_grasp_stride,
                                        int64_t R, int64_t K, double ds, int thresh, int32_t* profile, int32_t* result,
                                        void* stream);
int regnet_grasp_retreat_pick(const int32_t* result, int64_t B, int64_t R, int32_t* best, void* stream);
int64_t regnet_tsdf_sdf_workspace_bytes(int64_t nx, int64_t ny, int64_t nz, int sign, int with_nearest);
int regnet_tsdf_sdf(const void* volume, int64_t nx, int64_t ny, int64_t nz, double trunc, int64_t min_weight, double margin,
                    int mode, int outside, int sign, int64_t cap, int32_t* field, int32_t* nearest, void* work, void* stream);
int regnet_edt_metres_signed_f32(const int32_t* field, int64_t n, double voxel, float* out, void* stream);
int regnet_edt_query_signed_f32(const int32_t* field, const int32_t* nearest, int64_t nx, int64_t ny, int64_t nz,
                                const float* origin3, double voxel, const float* points, int64_t stride_row, int64_t stride_col,
                                int64_t M, const float* T12, int interpolate, float* distance, float* gradient,
                                float* nearest_xyz, void* stream);
int regnet_grasp_margin_volume_signed_f32(const int32_t* field, int64_t nx, int64_t ny, int64_t nz, const float* origin3,
                                          double voxel, int outside, const float* L, int64_t B, float x_lo, float x_hi,
                                          const float* x_hi_per_grasp, float half_thickness, float half_width, float half_space,
                                          float back_x, float standoff, double step, float x_extent, int32_t* margins,
                                          int32_t* counts, void* stream);
int regnet_edt_tile(int64_t n, int with_nearest);
int regnet_tsdf_edt(const void* volume, int64_t nx, int64_t ny, int64_t nz, double trunc, int64_t min_weight, double margin,
                    int mode, int outside, int32_t* dist2, int32_t* nearest, void* stream);
int regnet_tsdf_edt_pass(const void* volume, int64_t nx, int64_t ny, int64_t nz, double trunc, int64_t min_weight, double margin,
                         int mode, int outside, int pass, int32_t* dist2, int32_t* nearest, void* stream);
int regnet_edt_query_f32(const int32_t* dist2, const int32_t* nearest, int64_t nx, int64_t ny, int64_t nz, const float* origin3,
                         double voxel, const float* points, int64_t stride_row, int64_t stride_col, int64_t M, const float* T12,
                         float* distance, float* nearest_xyz, void* stream);
int regnet_edt_metres_f32(const int32_t* dist2, int64_t n, double voxel, float* out, void* stream);
int regnet_grasp_margin_volume_f32(const int32_t* dist2, int64_t nx, int64_t ny, int64_t nz, const float* origin3, double voxel,
                                   int outside, const float* L, int64_t B, float x_lo, float x_hi, const float* x_hi_per_grasp,
                                   float half_thickness, float half_width, float half_space, float back_x, float standoff,
                                   double step, float x_extent, int32_t* margins, int32_t* counts, void* stream);

/* ---- hand paths (csrc/hand_path.hip): posed trajectories of the hand against the distance field ---------------------------------
 * The retreat fan above translates the rigid hand at its final pose.  regnet_grasp_path_check_f32 /
 * regnet_grasp_path_check_signed_f32 (one kernel, a template parameter) take the POSE of the hand at every waypoint, so a path
 * may turn the hand as it moves.  field, dims, origin3 (HOST), voxel, outside, the box arguments, x_hi_per_grasp, step, x_extent
 * and thresh are the fan's and mean the same; canonical fp32 arithmetic as everywhere in this family.
 *   P           (B, R, K + 1, 12) float32 DEVICE: for grasp b, candidate path r and waypoint k the three rows of the hand's
 *               row-major LOCAL-TO-VOLUME matrix at that waypoint.  Waypoint 0 is the final grasp pose.  R in 1..16, K in 1..64.
 *   lattice     the fan's: the margin entries' with standoff = 0, hand samples only (back || finger for the grasp's own x_hi, a
 *               sample that is both counted once).  Membership is decided once per sample, in the hand's local frame.
 *   value       for every hand sample (x, y, z) and every k = 0 .. K: w = rows(b, r, k) applied by affine3 (csrc/common.h), the
 *               nearest voxel of w (csrc/hand_lattice.h: grid_voxel), the field word there.  An OUTSIDE sample contributes 0
 *               (signed: -1) under outside = 1 and nothing under outside = 0; a non-finite position (a NaN row) is OUTSIDE.
 *   profile     (B, R, K + 1) int32 or NULL: the minimum value over the hand samples at each waypoint, REGNET_EDT_NONE for an
 *               empty set.
 *   result      (B, R, 4) int32, the fan's layout byte for byte, so regnet_grasp_retreat_pick picks from it unchanged:
 *               { free_steps = the largest n in 0..K with profile[k] >= thresh for all 1 <= k <= n (waypoint 0 is not judged);
 *               the minimum of profile over waypoints 1..free_steps, REGNET_EDT_NONE when free_steps is 0; the minimum over
 *               waypoints 1..K; the number of OUTSIDE lookups over waypoints 1..K, whatever `outside` says }.
 *   disp        (B, R, K) float32 or NULL: disp[b, r, k] is the largest distance a point of the hand's bounding box moves from
 *               waypoint k to k + 1: the maximum (NaN when either operand is one), over the 8 corners c in {x_lo, x_hi of grasp
 *               b} x {-half_width, +half_width} x {-half_thickness, +half_thickness}, of sqrt(dot3(d, d)) with d_i = affine3(row
 *               i of waypoint k + 1, c) - affine3(row i of waypoint k, c): one float32 subtraction per component, dot3's order,
 *               a correctly rounded float32 root.  The displacement under a difference of two affine maps is convex in the
 *               point, so the maximum over the corners is the maximum over the box.
 * One workgroup of 256 threads per (grasp, path), the tile walk of the approach analysis; the path's rows are staged in LDS once.
 * The per-waypoint minima are LDS words lowered by LDS integer minima, the OUTSIDE count an integer sum: no floating-point sum,
 * no global atomic, no host read, no allocation; capturable; two runs give the same bytes.  Errors, all before the launch and in
 * the fan's order: B < 0, a dim < 1, outside not 0 / 1, R or K < 1 -> REGNET_ERR_SHAPE; a dim > 1024, N > 2^28, B >= 2^31, step
 * or voxel not finite or not positive (in float32 too), R > 16, K > 64, B R (K + 1) > 2^28, a lattice count that is not finite
 * or n_x n_y n_z > 2^22 -> REGNET_ERR_UNSUPPORTED; then B == 0: success without a launch; then a NULL field, origin3, P or result
 * -> REGNET_ERR_NULL.                                                                                                          */
int regnet_grasp_path_check_f32(const int32_t* field, int64_t nx, int64_t ny, int64_t nz, const float* origin3, double voxel,
                                int outside, const float* P, int64_t B, int64_t R, int64_t K, float x_lo, float x_hi,
                                const float* x_hi_per_grasp, float half_thickness, float half_width, float half_space,
                                float back_x, double step, float x_extent, int thresh, int32_t* profile, int32_t* result,
                                float* disp, void* stream);
int regnet_grasp_path_check_signed_f32(const int32_t* field, int64_t nx, int64_t ny, int64_t nz, const float* origin3,
                                       double voxel, int outside, const float* P, int64_t B, int64_t R, int64_t K, float x_lo,
                                       float x_hi, const float* x_hi_per_grasp, float half_thickness, float half_width,
                                       float half_space, float back_x, double step, float x_extent, int thresh, int32_t* profile,
                                       int32_t* result, float* disp, void* stream);

/* ---- push-out (csrc/hand_adjust.hip): a colliding hand moved free along the signed field's gradient ------------------------------
 * The margin, the fan and the paths judge a pose.  regnet_grasp_push_out_f32 MOVES the rigid hand of every grasp by a translation
 * until its interpolated signed margin reaches `target`; the rotation is kept.  Deepest-sample projection: at every iterate the
 * hand sample with the smallest interpolated signed distance is found, and the hand steps along the gradient there by the
 * distance that is missing.  field is the SIGNED plane (there is no unsigned twin: an unsigned field has no inside); dims,
 * origin3 (HOST), voxel, outside, L (B,12), the box arguments, x_hi_per_grasp, step and x_extent are the retreat fan's and mean
 * the same; canonical fp32 arithmetic as everywhere in this family.
 *   axes3       HOST, 3 float32: a factor per LOCAL axis (approach, closing, thickness) on the step; (1,1,1) moves freely,
 *               (0,1,0) along the closing axis only.
 *   target      metres, target_f = float32(target): the margin the hand is to reach.  max_shift: metres, cap2 = max_shift_f *
 *               max_shift_f, one float32 product.  T: the most steps, 1..64.
 *   samples     the fan's lattice (standoff = 0), HAND samples only (back || finger for the grasp's own x_hi, a sample that is
 *               both counted once), membership decided in the local frame.  The sample (i, j, k) has the linear index
 *               (i n_y + j) n_z + k.
 *   pose        at iterate n the rows are L's rotation and the translation t_i = (((r_i0 s_0) + (r_i1 s_1)) + (r_i2 s_2)) + t0_i
 *               = affine3(r_i0, r_i1, r_i2, t0_i, s) of the accumulated LOCAL shift s, recomputed from s at every applied step
 *               and never accumulated in the volume's frame.  While no step has been applied the rows are L's own, bit for bit.
 *   evaluate    for every hand sample w = affine3(row, x, y, z); an INSIDE sample (csrc/hand_lattice.h: grid_voxel) has the
 *               value of regnet_edt_query_signed_f32 with interpolate = 1 at w (csrc/sdf_sample.h).  A sample that is OUTSIDE
 *               or whose value is a NaN (infinite corners of an uncapped field) has no value and is counted as an OUTSIDE
 *               lookup.  The minimum is over the 64-bit keys (ordered(value) << 32) | index with ordered(v) = b ^ ((b >> 31) |
 *               0x80000000) of the value's bits b (an arithmetic shift): -0 sorts below +0, and of equal values the smallest
 *               index wins.  low = the winning value, +inf when no sample has one.
 *   decide      in this order, n the iterate:  1. no sample has a value and none was counted (the hand set is empty):
 *               ALREADY_FREE.  2. no sample has a value, or outside = 1 and any was counted: LEFT_VOLUME.  3. low >= target_f:
 *               ALREADY_FREE when n = 0, else FREED.  4. n == T: MAX_ITER.  5. g = the gradient of the interpolant at the worst
 *               sample (the volume's frame), a_k = axes_k * dot3(column k of the rotation, g), e = target_f - low, d_k = e *
 *               a_k, s'_k = s_k + d_k.  Any a_k a NaN, or d_0 == d_1 == d_2 == 0: STUCK.  !(dot3(s', s') <= cap2): CAPPED,
 *               and the step is NOT applied.  Otherwise s = s' and iterate n + 1 is evaluated.
 *   pose        (B,12) float32 DEVICE out: the final rows.  shift (B,3) float32: the local s.
 *   trace       (B, T + 1) float32 or NULL: low at every evaluated iterate, the NaN 0x7fc00000 at the others.
 *   info        (B,4) int32: { the status REGNET_PUSH_*, the steps applied, the worst sample's linear index at the last
 *               evaluation or -1 when none had a value, the OUTSIDE lookups at the last evaluation }.
 * One workgroup of 256 threads per grasp, the iteration inside the kernel, the tile walk of the approach analysis per iterate;
 * the keys are reduced by the wave butterfly and the four waves through LDS (a minimum has no order), the count is an integer
 * sum; every thread takes the same decision, so the exit is workgroup-uniform.  No floating-point sum, no global atomic, no host
 * read, no allocation; capturable; two runs give the same bytes.  Errors, all before the launch and in the fan's order: B < 0, a
 * dim < 1, outside not 0 / 1, T < 1 -> REGNET_ERR_SHAPE; a dim > 1024, N > 2^28, B >= 2^31, step or voxel not finite or not
 * positive (in float32 too), T > 64, target not finite in float32, max_shift negative or not finite in float32, a non-finite
 * axes3 (where it is given), a lattice count that is not finite or n_x n_y n_z > 2^22 -> REGNET_ERR_UNSUPPORTED; then B == 0:
 * success without a launch; then a NULL field, origin3, L, axes3, pose, shift or info -> REGNET_ERR_NULL.                        */
#define REGNET_PUSH_ALREADY_FREE 0
#define REGNET_PUSH_FREED 1
#define REGNET_PUSH_MAX_ITER 2
#define REGNET_PUSH_CAPPED 3
#define REGNET_PUSH_STUCK 4
#define REGNET_PUSH_LEFT_VOLUME 5
int regnet_grasp_push_out_f32(const int32_t* field, int64_t nx, int64_t ny, int64_t nz, const float* origin3, double voxel,
                              int outside, const float* L, int64_t B, float x_lo, float x_hi, const float* x_hi_per_grasp,
                              float half_thickness, float half_width, float half_space, float back_x, double step,
                              float x_extent, const float* axes3, double target, double max_shift, int64_t T, float* pose,
                              float* shift, float* trace, int32_t* info, void* stream);

/* ---- next-best view (csrc/view_gain.hip): which candidate camera pose reveals the most of the space no view has observed --------
 * The approach analysis above reports the unobserved space a grasp's hand sweeps through; these entry points say where a camera
 * should go so that it becomes observed.  Integer results only; canonical fp32 arithmetic (individually rounded binary32
 * operations in the written order, -ffp-contract=off, __fdiv_rn, strict comparisons) decides which voxel a ray's sample falls in.
 * The volume is only read.  tests/view_gain_reference.py restates all three.
 *
 * regnet_tsdf_view_mark_f32: per candidate pose, the UNKNOWN voxels its rays reach.
 *   volume, dims, origin3 (3 float32, HOST), voxel, trunc, min_weight, margin   as for regnet_grasp_approach_volume_f32:
 *               voxel_f = float32(voxel), d_solid = float32(margin / trunc), the division in float64, rounded once.
 *   intrinsics4 (4 float32, HOST), near, step, n_steps, width, height, clip   as for regnet_tsdf_raycast_f32.
 *   poses       (P,12) float32 DEVICE: per candidate rows 0..2 of the row-major 4x4 CAMERA-TO-COMMON transform.  1 <= P <= 32.
 *   ray point   of pixel (u, v) of pose p at sample i: regnet_tsdf_raycast_f32's.  z_i = near_f + ((float)i * step_f); c_x =
 *               (((float)u - cx) * z) * rfx, c_y = (((float)v - cy) * z) * rfy, c_z = z; w_k = (((r_k0 c_x) + (r_k1 c_y)) + (r_k2
 *               c_z)) + t_k with pose p's rows.
 *   lookup      regnet_grasp_approach_volume_f32's: per axis c = floorf(__fdiv_rn(w - o, voxel_f)), INSIDE iff c >= 0 && c <
 *               (float)n on all three axes, compared in float; the NEAREST voxel l, nothing interpolated.
 *   class       regnet_grasp_approach_volume_f32's OUTSIDE / UNKNOWN / SOLID / FREE (one definition, csrc/hand_lattice.h).
 *   march       over i ascending.  OUTSIDE or FREE: go on.  SOLID: the ray ends BLOCKED.  UNKNOWN at voxel l: when interest is
 *               NULL or interest[l] != 0, bit p of plane[l] is set (a bit REQUEST); whether or not, the ray's count of unknown
 *               samples goes up by one, and when it reaches max_unknown (1 .. n_steps) the ray ends SATURATED: a camera does not
 *               see through that much unobserved matter.  Consecutive samples in one voxel each count.  A ray that ends neither
 *               way: EXITED.
 *   interest    (N) uint8 DEVICE or NULL: the voxels whose observation is wanted.
 * Outputs, DEVICE memory: plane (N) uint32, N = nx ny nz: cleared by a fill on the stream, then bit p of word l set iff a ray of
 * pose p requested it (an integer atomic OR; a plain load first skips the atomic when the bit is already there, which cannot
 * change the result: bits are only set); status (P, height width) uint8 or NULL: 0 EXITED, 1 BLOCKED, 2 SATURATED, row v width +
 * u; rays (P,4) int32: the histogram of status and, in column 3, the rays with at least one bit request (a request counts even
 * when the bit was already set), cleared by a fill, then collected in LDS with one integer atomic per workgroup and column.
 * Grid z is the pose; 16 x 16 pixels per 256-thread workgroup, an 8 x 8 tile per wave.  clip as for the raycast (the same
 * float64 slab test, csrc/ray_clip.h: the samples it leaves out are OUTSIDE): it changes the time and no bit.  Three launches
 * (the two fills are kernels); no host read, no synchronisation, no allocation, no floating-point atomic: capturable.  Errors, all before any
 * launch: a dim, P, width, height, n_steps, min_weight or max_unknown < 1 -> REGNET_ERR_SHAPE; P > 32, max_unknown > n_steps, a
 * dim > 2^24, N > 2^28, min_weight >= 2^31, width height > 2^21, n_steps > 4096, voxel, trunc, near or step not finite or not
 * positive (in float32 too), margin / trunc not finite in float32 -> REGNET_ERR_UNSUPPORTED; a NULL volume, origin3,
 * intrinsics4, poses, plane or rays -> REGNET_ERR_NULL.
 *
 * regnet_tsdf_view_pick: the greedy JOINT selection of K of the P poses of a plane, so that the second pick adds what the first
 * does not cover.  gain (P) int32: per pose the number of words with its bit set.  Round r = 0 .. K - 1: per pose the number of
 * words with its bit set and NO bit of an already chosen pose; the largest count wins, the lowest index among equals;
 * order[r] = that pose, order_gain[r] = its count, and the pose joins the chosen ones.  When the best count is < max(min_gain, 1)
 * this and every later round write order = -1, order_gain = 0.  state: REGNET_VIEW_PICK_STATE_WORDS int32 of DEVICE scratch (the
 * chosen mask, the stop flag, the round's counts), cleared by a fill.  Per round a counting launch over the plane (wave ballots
 * and population counts; one integer atomic per workgroup and pose) and a one-workgroup decision launch: 2 K + 1
 * launches with the fill, no host read: capturable.  Integer sums only, so the result has no order.  Errors: N, P or K < 1 or min_gain < 0 ->
 * REGNET_ERR_SHAPE; N > 2^28, P > 32 or K > P -> REGNET_ERR_UNSUPPORTED; a NULL pointer -> REGNET_ERR_NULL.
 *
 * regnet_tsdf_view_interest_hands: the interest plane of the swept hands of B grasps.  The arguments up to x_extent, the lattice,
 * the sets and the lookup are regnet_grasp_approach_volume_f32's.  For every looked-up sample (region, hand or blocker) whose
 * voxel is UNKNOWN, interest[l] = 1: a plain byte store of the same value from every writer, no atomic.  OUTSIDE samples have no
 * voxel and store nothing.  The caller clears interest (N) uint8.  counts (B) int32: the UNKNOWN samples per grasp, an integer
 * sum (a sample counts once, whatever its hand membership).  One launch, one workgroup of 256 threads per grasp; capturable.
 * Errors: regnet_grasp_approach_volume_f32's, with interest and counts the required outputs.                                 */
#define REGNET_VIEW_PICK_STATE_WORDS 64
int regnet_tsdf_view_mark_f32(const void* volume, int64_t nx, int64_t ny, int64_t nz, const float* origin3, double voxel,
                              double trunc, int64_t min_weight, double margin, const float* intrinsics4, const float* poses,
                              int64_t P, double near, double step, int64_t n_steps, int64_t width, int64_t height, int clip,
                              int64_t max_unknown, const uint8_t* interest, uint32_t* plane, uint8_t* status, int32_t* rays,
                              void* stream);
int regnet_tsdf_view_pick(const uint32_t* plane, int64_t N, int64_t P, int64_t K, int64_t min_gain, int32_t* state, int32_t* gain,
                          int32_t* order, int32_t* order_gain, void* stream);
int regnet_tsdf_view_interest_hands(const void* volume, int64_t nx, int64_t ny, int64_t nz, const float* origin3, double voxel,
                                    double trunc, int64_t min_weight, double margin, const float* L, int64_t B, float x_lo,
                                    float x_hi, const float* x_hi_per_grasp, float half_thickness, float half_width,
                                    float half_space, float back_x, float standoff, double step, float x_extent,
                                    uint8_t* interest, int32_t* counts, void* stream);

/* ---- deterministic mode (csrc/scatter.hip, csrc/det.hip, csrc/bn_train.hip) ------------------------------------------
 * The float32 kernels behind torch.use_deterministic_algorithms(True): every sum of the training backward is formed in one
 * fixed order, so runs agree bit for bit.  The default entry points above are unchanged.
 *   - regnet_scatter_plan: the per-scene sort plan of a destination table index (B, num_src) int64 contiguous (source
 *     position p of scene b -> destination index[b, p]; outside [0, num_dest): no destination) into `plan`, of
 *     regnet_scatter_plan_bytes(B, num_dest, num_src) bytes, 16-byte aligned: the source positions of every destination in
 *     ascending order.  It depends on the indices alone; build it once per table and hand it to every segment sum of it.
 *   - regnet_scatter_segsum_f32: grad_in (B, C, num_dest) contiguous, written whole, = per destination the sum of its
 *     contributions in ascending source position, sequentially from +0.0 (np.add.at on float32 arrays).  Unweighted
 *     (weight NULL, group_points / gather_knn): p = row * inner + k, the value grad_out[b*sb + c*sc + row*s_hi + k*s_lo].
 *     Weighted (interpolate, inner must be 3, s_lo unused): weight (B, num_src) contiguous, the value is the float32
 *     product grad_out[b*sb + c*sc + (p/3)*s_hi] * weight[b, p].  `plan` built from the same index and sizes.
 *   - regnet_scatter_max_grad_det_f32: regnet_scatter_max_grad_f32 with the additions to every destination in ascending r,
 *     onto the value already there.  R <= 8192 (else REGNET_ERR_UNSUPPORTED).
 *   - regnet_bn_*_det_f32: the training BatchNorm entry points with per-workgroup partials added in a fixed order instead
 *     of float atomics; workspace of regnet_bn_det_workspace_bytes(B, C, L) bytes.                                        */
int64_t regnet_scatter_plan_bytes(int64_t B, int64_t num_dest, int64_t num_src);
int regnet_scatter_plan(const int64_t* index, int64_t B, int64_t num_dest, int64_t num_src, void* plan, void* stream);
int regnet_scatter_segsum_f32(const float* grad_out, int64_t sb, int64_t sc, int64_t s_hi, int64_t s_lo, int64_t inner,
                              const float* weight, int64_t B, int64_t C, int64_t num_dest, int64_t num_src, const void* plan,
                              float* grad_in, void* stream);
/* regnet_scatter_segsum_route / regnet_scatter_atomic_route: HOST code, no device and no stream -- which kernel the backwards of
 * group_points / gather_knn / interpolate take for B scenes, C channels, num_dest destinations and num_src sources per scene
 * (the launchers call the same functions).  route is host memory.
 *   regnet_scatter_segsum_route: the segment sums of regnet_scatter_segsum_f32 (elem_size 4) and of the float64 backwards
 *     (elem_size 8); weighted != 0 for interpolate (num_src = N * 3).  route (3 int64):
 *       [0] 1 segsum_lds_kernel with every source slot staged at once, 2 segsum_lds_kernel over several chunks of slots,
 *           3 segsum_global_kernel, 0 no segment-sum kernel (an empty size, or unsupported);
 *       [1] channels per workgroup (1, 2) or per thread (3);  [2] slots per chunk (1, 2), 0 for the global kernel.
 *   regnet_scatter_atomic_route: the default float32 backwards (regnet_group_points_bwd_f32, regnet_gather_knn_bwd_f32:
 *     num_src = N2 * K; regnet_interpolate_bwd_f32: num_src = N).  route (2 int64):
 *       [0] 1 scatter_add_lds_kernel (LDS atomics), 2 zero fill + the global-atomic kernel, 0 no kernel (num_src == 0: zero
 *           fill alone; or unsupported);   [1] channels per workgroup.
 * Return REGNET_OK, or REGNET_ERR_UNSUPPORTED exactly where the launcher returns it for these sizes (route zeroed),
 * REGNET_ERR_SHAPE (negative size, elem_size not 4 or 8, weighted with num_src % 3 != 0), REGNET_ERR_NULL (route == NULL).  */
int regnet_scatter_segsum_route(int elem_size, int weighted, int64_t B, int64_t C, int64_t num_dest, int64_t num_src,
                                int64_t* route);
int regnet_scatter_atomic_route(int64_t B, int64_t C, int64_t num_dest, int64_t num_src, int64_t* route);
int regnet_scatter_max_grad_det_f32(const float* dy, const int64_t* arg, int64_t R, int64_t F, int64_t scene_rows,
                                    int64_t batch_stride, int64_t row_stride, int64_t ch_stride, float* grad, void* stream);
int64_t regnet_bn_det_workspace_bytes(int64_t B, int64_t C, int64_t L);
int regnet_bn_relu_train_fwd_det_f32(const float* x, int64_t B, int64_t C, int64_t L, const float* gamma, const float* beta,
                                     float eps, float momentum, float* running_mean, float* running_var, int relu,
                                     int64_t pool_group, float* y, int32_t* pool_index, float* save_mean, float* save_invstd,
                                     void* workspace, void* stream);
int regnet_bn_relu_train_bwd_det_f32(const float* x, const float* y, const float* dy, const int32_t* pool_index, int64_t B,
                                     int64_t C, int64_t L, const float* gamma, const float* beta, const float* save_mean,
                                     const float* save_invstd, int relu, int64_t pool_group, float* dx, float* dgamma,
                                     float* dbeta, void* workspace, void* stream);
int regnet_bn_train_stats_det_f32(const float* x, int64_t B, int64_t C, int64_t L, const float* gamma, const float* beta,
                                  float eps, float momentum, float* running_mean, float* running_var, float* save_mean,
                                  float* save_invstd, float* scale, float* shift, void* workspace, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* REGNET_HIP_H_ */
