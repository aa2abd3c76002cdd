/*
 * lio_hip.h -- C ABI of the MI355X-native LIO scan-matching core (liblio_hip.so).
 *
 * This is the drop-in boundary for ONE hot path of w111liang222/lidar-slam-detection:
 * the per-scan  voxel-grid downsample -> map kNN -> point-to-plane residual + Jacobian
 * accumulation -> iterated ESKF update -> map insert  loop of the FastLIO frontend, and
 * the callers either side of it:
 *   lio_map_* / lio_scan_* / lio_p2plane_* ... the kernels' level (iVox, VoxelGrid, h_share_model)
 *   lio_engine_* ........................... fastlio_main after IMU processing, the 23-DoF filter
 *   lio_fastlio_* .......................... the reference's FastLIO entry points one to one (IMU front half included)
 *   lio_engines_process_batch, lio_engine_set_reduce_hook ... throughput mode, joint registration across GPUs
 *   lio_ndt_* / lio_pose_estimator_* / lio_localmap_* ........ the localisation mode's matcher, its filter, its local map
 *   lio_state_* / lio_eskf_update_cb ....... host-only helpers that pin the filter algebra
 * Every entry point names the reference interface it replaces (paths relative to
 * /root/reference/slam/mapping/fastlio unless stated otherwise).
 *
 * Conventions
 *   - plain C, opaque handles, caller-owned buffers, no exceptions cross the ABI;
 *   - return value: >= 0 ok (often a count), < 0 one of LIO_E_*;
 *   - points are XYZI float quadruples (16 B, "float4"); quaternions are (x, y, z, w);
 *   - "_device" variants take pointers that are already resident in HBM on the handle's
 *     device (e.g. a torch tensor's data_ptr()); the others take host pointers;
 *   - a handle owns one HIP stream; a handle is not thread-safe; distinct handles may be
 *     driven from distinct host threads / on distinct GPUs.
 *   - there is NO CPU fallback: without a usable HIP device every create() returns NULL.
 */
#ifndef LIO_HIP_H_
#define LIO_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LIO_OK 0
#define LIO_E_INVALID (-1)     /* bad argument / handle */
#define LIO_E_CAPACITY (-2)    /* a fixed capacity (points, voxels, ds points) would be exceeded */
#define LIO_E_DEVICE (-3)      /* HIP runtime error (message via lio_last_error) */
#define LIO_E_STATE (-4)       /* call order violated (e.g. linearize before a scan is set) */

typedef struct lio_map lio_map;       /* iVox-equivalent hash-grid map resident in HBM */
typedef struct lio_scan lio_scan;     /* one scan in flight: raw, downsampled, neighbour cache, gates */
typedef struct lio_engine lio_engine; /* per-scan driver = the body of fastlio_main after IMU processing */

const char* lio_last_error(void);
/* notes of calls that SUCCEEDED (thread-local, like lio_last_error, which only failures write): e.g. lio_batch_create when GPU_MAX_HW_QUEUES
 * leaves its rounds in flight sharing hardware queues */
const char* lio_last_warning(void);
int lio_device_count(void);
/* The ABI revision this header describes; lio_abi_version() returns the revision the loaded library was built from.  A caller built against an
 * older header can keep running as long as it checks that the library's revision is >= its own: revisions only APPEND (struct tails, flag bits,
 * entry points).  History: 4 = round 4 (lio_batch_times grew by insert_us / insert_launches / pad: a caller that allocates the round-3 struct and
 * calls a revision-4 library is written past -- rebuild, or check the revision and allocate sizeof(lio_batch_times) of THIS header;
 * lio_timings.n_added may be -1 = "insert still in flight, not read back"; lio_engine_timings may return a deferred LIO_E_CAPACITY);
 * 5 = round 5 (LIO_JOB_HOST_RAW, lio_pinned_alloc / lio_pinned_free, lio_abi_version itself);
 * 6 = round 6 (lio_map_set_tie_mode / lio_map_tie_stats: candidates exactly as far as the fifth nearest are now kept as the reference keeps them);
 * 7 = lio_cloud_* (the dense-map export: a device-resident cloud that grows over a drive, and the VoxelGrid of the whole cloud);
 * 8 = lio_knn_index_* (exact k nearest neighbours over a static cloud; texture_mesh);
 * 9 = lio_ground_* (the ground detector: height clip, normals, plane RANSAC, inlier cloud);
 * 10 = lio_bev_* (the bird's-eye intensity image of a dense map: noise filter, per-pixel means, patch equalisation, 16-bit image);
 * 11 = lio_keyframe_* / lio_keyframer_* / lio_radius_outlier_host (the mapping mode's key frames: decision, fitness against a rolling local map,
 * election, radius outlier and range filters);
 * 12 = lio_loop_* (loop detection over the key frames: candidate search, batched FAST_VGICP with the LM loop on the device, nearest-neighbour
 * fitness, FAST_GICP verification, the loop edge with its information matrix);
 * 13 = lio_graph_* / lio_se3_* / lio_loop_pair_information (the pose graph: SE3 edges, Huber, Levenberg-Marquardt with a conjugate-gradient solve
 * on the device; the information matrix of two bank frames under a relative pose);
 * 14 = lio_scan_undistort_imu (test visibility: the FastLIO front half's point filter and IMU backward propagation on caller-supplied poses).
 * 15 = lio_graph_add_prior / set_kernel / priors / prior_error / remove_gnss_outliers, LIO_GRAPH_KERNEL_DCS2 (the pose graph's unary edges: GNSS
 *      position, orientation and floor-plane priors, the DCS2 kernel, the GNSS outlier stage of robust_graph_optimize).
 * 16 = lio_overlap_* (overlap detection between two maps over a lio_loop bank: candidate search over the graph's connections, the range-gated
 *      fitness for many pairs, FAST_VGICP for arbitrary (target, source) pairs in one set of rounds, the fine target accumulated on the device,
 *      one detect() call over a fragment of new key frames).
 * 17 = lio_gicp_neighbours / lio_gicp_mahalanobis (test visibility: the neighbour list behind every covariance, the Mahalanobis matrices of the
 *      current pairs).  lio_gicp_set_target / _set_source now refuse points that are not finite, lio_gicp_linearize / _align a pose that is not
 *      finite or a max_corr_dist that is negative or NaN (LIO_E_INVALID, nothing launched, the object as it was).
 * 18 = lio_sc_* (the Scan Context bank of the relocalisation: descriptors of many clouds in one set of launches, the ring-key search, the
 *      column-shift distance, globalSearch) and lio_gicp_fitness_score (getFitnessScore of the handle's own pair).
 * 19 = lio_gicp_set_target_device / _set_source_device (a cloud in HBM through the host entry's path), lio_scan_ds_device, lio_localmap_nearest /
 *      _gather / _z_mean / _download_gather / _gather_device / _store_frame / _frame / _estimate_pose, lio_estimate_matcher_params (the operator's
 *      pose hint, GlobalLocalization::getEstimatePose, on the device).  lio_gicp_set_target / _set_source now leave the cloud in an internal
 *      order that is a function of the cloud (it was the grid's arrival order: lio_gicp_download differed from call to call, T in its last bits).
 * 20 = lio_render_* (the road-surface colour map of slam/localization/map_render: voxels of floor points painted from camera images -- insert,
 *      projection, z-buffer, depth continuity, bilinear sample, running blend, export).
 * 21 = lio_graph_remove_node, lio_graph_node_live, lio_graph_edge_records, lio_loop_retire (a key frame leaves the map: graph_del_vertex; and
 *      the graph hands back its edges as they were added: graph_save).  A removed node's id, and a retired frame's, is refused as unknown.
 * 22 = lio_utm_* / lio_grid_convergence / lio_transform_from_rpyt / lio_quat_of_transform / lio_interpolate_transform / lio_rtk_transform_* /
 *      lio_rtk_track_* / lio_gnss_queue_* (the GNSS side of mapping mode on the host: UTM projection, the RTK track of RTKM, the graph's GNSS
 *      queue) and lio_scan_merge_* (several lidars into one frame on the device: mergePoints + preprocessPoints).
 * 23 = lio_sc_set_positions / lio_sc_local_search (the INS-aided start of the relocalisation: GlobalLocalization::localSearch over the key
 *      frames' positions resident beside the descriptors) and lio_update_origin (a map's poses and GNSS priors under another origin).
 * 24 = lio_calib_* / lio_se3f_* / lio_dfo_* (the lidar-INS calibration: Scan's subsampling, the f32 Transform, the odometry interpolation and
 *      two derivative-free minimisers on the host; the capped k-NN cost of all key scans and Aligner::lidarOdomTransform on the device).
 * 25 = lio_graph_estimate_gnss_moment / lio_graph_moment_begin / _end / _get / _linearize (the GNSS moment stage of robust_graph_optimize's mode
 *      `mapping`: one shared 3-DoF vertex, the offset between the antenna and the lidar frame, bordered onto the pose graph's system).
 * 26 = lio_calib_ground_* (the lidar ground calibration: the polygon crop, fit_plane's RANSAC scored a batch of planes per pass over the
 *      points, the loop replayed on the host).
 * 27 = lio_calib_imu_* (the lidar-IMU calibration: gyro integration, time alignment and the quaternion hand-eye solve on the host; the tool's
 *      own lidar odometry -- voxel filter, FAST_VGICP against a local map that stays in HBM -- on the device).
 * 28 = lio_boxes_* (detection boxes: rotated BEV overlap, convex hull area, BEV IoU and GIoU3D of box pairs, rotated NMS with the sweep on
 *      the device, and the detector's post-process -- filter, order, NMS, gather -- as one call).
 * 29 = lio_voxelizer_* / lio_voxelize_grid_size (the detection front end: the sliding window of sweeps, the hash voxeliser and the mean VFE to
 *      f16, pinned to the reference's kernels run one thread after another in index order). */
#define LIO_ABI_VERSION 29
int lio_abi_version(void);
/* page-locked host memory for clouds handed over with LIO_JOB_HOST_RAW (or lio_scan_upload): copies from it run at the link's rate and
 * overlap with kernels; NULL on failure.  Any hipHostMalloc'ed / hipHostRegister'ed range serves as well. */
void* lio_pinned_alloc(uint64_t bytes);
void lio_pinned_free(void* p);
/* bytes of HBM currently held by a map / scan handle (capacity planning on the 288 GB part) */
uint64_t lio_map_bytes(const lio_map*);

/* ---------------------------------------------------------------------------------------------
 * Map: replaces faster_lio::IVox<3, DEFAULT, PointType>  (include/ivox3d/ivox3d.h:59-120)
 *   voxel key = round-half-away(p / resolution) per axis (ivox3d.h:258-261)
 *   stencils  = 1 (CENTER), 7 (NEARBY6), 19 (NEARBY18), 27 (NEARBY26), 75 ("NEARBY74", 5x5x3)
 *               (ivox3d.h:179-210)
 * ------------------------------------------------------------------------------------------- */
/* ctor: IVox(Options) as configured at src/laserMapping.cpp:1060-1064.  max_points bounds the point
 * pool (the pool is 2x that to leave slack for voxel growth), max_voxels the number of live voxels. */
lio_map* lio_map_create(int device, float resolution, uint64_t max_points, uint64_t max_voxels, int stencil);
void lio_map_destroy(lio_map*);
/* IVox::SetNearByType (used at src/laserMapping.cpp:1241-1243) */
int lio_map_set_stencil(lio_map*, int stencil);
/* IVox::AddPoints(points, travel_distance)  (ivox3d.h:231-256).  Points are appended to their voxels;
 * new voxels are stamped with `travel`.  The LRU list of the reference (least recently touched voxel dropped
 * above `capacity` voxels once it is older than `max_distance`) is opt-in: lio_map_set_lru below; without it
 * nothing is ever dropped and exceeding max_points / max_voxels returns LIO_E_CAPACITY. */
int lio_map_insert(lio_map*, const float* world_xyzi, uint64_t n, double travel);
int lio_map_insert_device(lio_map*, const void* d_world_xyzi, uint64_t n, double travel);
/* back to an empty map without giving its memory back: what `ivox = std::make_shared<IVoxType>(ivox_options)` does in fastlio_init (src/laserMapping.cpp:1064) when the
 * reference starts over -- here also the way a checker puts a map of known content in place (clear, then one lio_map_insert of that content: points of a
 * voxel keep the order of the inserted array, as IVoxNode::InsertPoint's push_back does).  The LRU list, if on, starts over with the map. */
int lio_map_clear(lio_map*);
/* IVox::Options capacity_ / max_distance_ (ivox3d.h:46-52; 100000 voxels / 100 m at src/laserMapping.cpp:1060-1064): turn
 * on the LRU list of IVox::AddPoints (ivox3d.h:231-256) -- after every inserted point the least recently touched voxel is
 * dropped while the map holds more than `capacity_voxels` voxels and that voxel was created more than `max_distance` of
 * travel ago.  Call before the first insert; `max_voxels` of lio_map_create stays the hard limit and must be larger (the map
 * overshoots its capacity while nothing is old enough to go).  Off by default (nothing is ever dropped).
 * lio_map_lru_stats: voxels evicted so far, and an UPPER BOUND on the back-of-list voxels that were touched by the very
 * batch that was evicting around them.  If such a voxel's first point of the batch comes after its turn to go, the reference's
 * point-by-point order drops it and creates it again holding the batch's points alone: since ABI revision 6 so does the device
 * (the pops of a batch are replayed in order, csrc/hashmap.hip lru_exact_*; LIO_LRU_EXACT=0 in the environment when the map is
 * made: counted only, the voxel keeps its points).  lio_map_lru_exact_stats: voxels dropped and re-created that way, and the
 * batches in which the order could not be followed -- the map above its capacity before the batch, or a voxel younger than
 * max_distance at the back of the list, where pops no longer coincide with creations -- and the batch was handled as a whole. */
int lio_map_set_lru(lio_map*, uint64_t capacity_voxels, double max_distance);
int lio_map_lru_stats(lio_map*, uint64_t* n_evicted, uint64_t* n_interleaved);
int lio_map_lru_exact_stats(lio_map*, uint64_t* n_recreated, uint64_t* n_batches_not_followed);
/* Which five, when the fifth and the sixth nearest candidate of a query are EXACTLY equally far (f32 d2).  IVox::GetClosestPoint cuts every stencil
 * voxel's in-range points to five and then the whole list to five with std::nth_element on the distance alone (ivox3d_node.hpp:107-127,
 * ivox3d.h:156-164): which of the equally distant candidates survives is what libstdc++'s introselect does to that particular sequence (stencil
 * order, push_back order inside a voxel).  mode 1 (default): the same survivor -- the map keeps every point's push_back rank, and the exact redo
 * of tied queries runs the same selection on the same sequence (csrc/refsel.h); mode 0: the five smallest in (d2, x, y, z), the definition of
 * rounds 1-5.  The two differ only on such ties (about one query in 1e6 on sensor data); the returned lists are in the canonical order either way.
 * mode 2: the lists exactly as the reference returns them, ORDER included (nearest first, the rest as introselect leaves them) -- every query of
 * every search is redone by the reference's selection, tens of times slower than the search itself: a parity mode (the plane fit's QR sees its rows
 * in the reference's order, so the whole path follows the reference's build to the rounding of the f64 sums), not a production mode.
 * lio_map_tie_stats: queries whose set the selection decided so far, and how many of those could not be resolved (a stencil voxel of more
 * than 2560 points: the canonical set was kept) -- 0 unless a map holds voxels of thousands of points. */
int lio_map_set_tie_mode(lio_map*, int mode);
int lio_map_tie_stats(lio_map*, uint64_t* n_boundary_ties, uint64_t* n_unresolved);
/* capacity planning: slots of the point pool handed out so far by the bump allocator (recycled regions of evicted / outgrown
 * voxels are re-used first and do not move it) and the pool's size, both in points of 16 B */
int lio_map_pool_stats(lio_map*, uint64_t* pool_top, uint64_t* pool_cap);
/* IVox::NumValidGrids (ivox3d.h:173-176) and the total number of stored points */
int lio_map_stats(lio_map*, uint64_t* n_points, uint64_t* n_voxels);
/* running total of map points visited by stencil kNN queries (the C-bar * N_ds statistic of the roofline model) */
uint64_t lio_map_knn_candidates(lio_map*);
/* running total of map points whose 16 bytes the kNN sweep actually asked for (it prunes stencil voxels that cannot hold one of the five
 * nearest, exactly) -- counted only by the diagnostic kernel variant that lio_batch_enable_kernel_timing(b, 2) selects; 0 otherwise */
uint64_t lio_map_knn_touched(lio_map*);
/* ... and of those the DISTINCT ones per launch, summed over the counted launches (a bitmap over the point pool, cleared before every counted launch):
 * the bytes a launch cannot avoid moving once -- 16 B for every distinct candidate point -- whatever its caches do */
uint64_t lio_map_knn_unique(lio_map*);
/* all stored points, voxel by voxel in unspecified order; returns the count or -(needed) */
int64_t lio_map_dump(lio_map*, float* out_xyzi, uint64_t cap_points);
/* IVox::GetClosestPoint(pt, out, 5, 5.0) for a batch of world-frame queries (ivox3d.h:139-171):
 * out_pts is n x 5 x 4 floats -- the reference's five (lio_map_set_tie_mode) in the canonical order (d2, x, y, z) ascending, out_cnt[n] the number
 * found (0..5).  Test/diagnostic entry; the per-scan path uses lio_p2plane_linearize. */
int lio_map_knn(lio_map*, const float* world_xyzi, uint32_t n, float* out_pts, int32_t* out_cnt);

/* ---------------------------------------------------------------------------------------------
 * Scan: replaces the file-scope per-scan buffers feats_undistort / feats_down_body /
 * feats_down_world / Nearest_Points / point_selected_surf / normvec / res_last
 * (src/laserMapping.cpp:86-124) and downSizeFilterSurf (src/laserMapping.cpp:127,1206-1207).
 * The neighbour cache persists across scans exactly like Nearest_Points does.
 * ------------------------------------------------------------------------------------------- */
lio_scan* lio_scan_create(int device, uint32_t max_raw, uint32_t max_ds);
void lio_scan_destroy(lio_scan*);
/* forget the neighbour cache and gate flags, as fastlio_init() does for Nearest_Points / point_selected_surf
 * (src/laserMapping.cpp:1045-1047) */
int lio_scan_reset(lio_scan*);
int lio_scan_upload(lio_scan*, const float* body_xyzi, uint32_t n_raw);          /* host -> HBM */
int lio_scan_set_device(lio_scan*, const void* d_body_xyzi, uint32_t n_raw);     /* already in HBM (not copied) */
/* pcl::VoxelGrid<PointType>::filter with setLeafSize(leaf, leaf, leaf) (PCL 1.9.1 voxel_grid.hpp,
 * called at src/laserMapping.cpp:1206-1207): centroid of every occupied voxel, ascending voxel index.
 * Asynchronous; *n_ds (may be NULL) is only filled when sync != 0. */
/* undistortPoints(const Eigen::Matrix4f& delta_pose, PointCloudAttrPtr&, double scan_period)   slam/common/slam_utils.cpp:163-191,
 * called by the localisation mode before the downsample (hdl_localization_nodelet.cpp:224-227) with delta_pose = start^-1 * stop of the
 * filter's prediction: constant-velocity motion compensation of the uploaded cloud, p' = Exp(r * log(delta)) p with r = stamp / period,
 * all in f32 as there.  delta_pose is row-major; stamp_us[i] is PointAttr::stamp (us from the scan start), a host array
 * (stamps_on_device = 0) or a device array.  Runs on the scan's stream; the result replaces the scan's raw cloud (a caller-owned
 * device cloud given by lio_scan_set_device is not written).  lio_scan_download_raw returns the point count. */
int lio_scan_undistort_delta(lio_scan*, const uint32_t* stamp_us, int stamps_on_device, const float delta_pose[16], double scan_period);
int lio_scan_download_raw(lio_scan*, float* out_xyzi, uint32_t cap);
/* undistortPoints(std::vector<PoseType>& poses, PointCloudAttrPtr&)   slam/common/slam_utils.cpp:193-228 (graph back end and map export: the
 * cloud compensated with a LIST of poses, e.g. the IMU poses of a frame): poses[i] = (absolute stamp us, motion T since poses[0], row-major
 * 4 x 4), i = 0 is the scan start; a point uses the first pose interval, from the one its predecessor used onwards, that ends
 * (pose_stamp[i] - header_stamp, unsigned) not before its stamp; points past the last pose, and everything after them, are left alone.
 * The interval ends must not decrease (LIO_E_INVALID otherwise); at most 64 poses. */
int lio_scan_undistort_poses(lio_scan*, const uint32_t* stamp_us, int stamps_on_device, uint64_t header_stamp_us, const uint64_t* pose_stamp_us,
                             const double* pose_T, uint32_t n_poses);
/* test visibility for the front half: Preprocess::velodyne_handler's point filter and ImuProcess::UndistortPcl's backward propagation
 * (preprocess.cpp:395-451, IMU_Processing.hpp:371-404) on the uploaded cloud with CALLER-SUPPLIED IMU poses -- the very launcher and kernels
 * lio_fastlio_main runs after its forward propagation, without the filter state in between.  poses: n_poses x 22 doubles, each
 * (offset_time s, acc[3], gyr[3], vel[3], pos[3], R[9] row-major), offsets not decreasing, poses[0] the scan start; end_pos3 /
 * end_rot_xyzw / ril_xyzw / til3: position, attitude and lidar-IMU extrinsics of the state at the scan end; a point whose f32
 * x*x + y*y + z*z is not above blind^2, or whose index is no multiple of filter_num (> 1), becomes NaN (intensity kept); undistort = 0:
 * the filters alone (stamps, poses and the end state are not read and may be NULL).  stamp_us as for lio_scan_undistort_delta, staged in
 * the downsample's second key buffer; the per-workgroup minima of the kernel go to its first key buffer (2 words per 256 points; both
 * are free until lio_scan_voxel_downsample runs on the same stream); the pose table is uploaded per call.  n_poses outside 2..128 with
 * undistort on: LIO_E_CAPACITY, the cloud is left as it was.  Waits for the result; it replaces the scan's raw cloud as
 * lio_scan_undistort_delta's does. */
int lio_scan_undistort_imu(lio_scan*, const uint32_t* stamp_us, int stamps_on_device, const double* poses, uint32_t n_poses, const double* end_pos3,
                           const double* end_rot_xyzw, const double* ril_xyzw, const double* til3, double blind, int filter_num, int undistort);
int lio_scan_voxel_downsample(lio_scan*, float leaf, int sync, uint32_t* n_ds);
/* the same filter over n scans (each holding its raw cloud: lio_scan_upload / lio_scan_set_device) with ONE set of launches -- the batched
 * chain of lio_batch, blockIdx.y = scan -- for callers that hold many clouds at once (the candidate key frames of the map-merge tools,
 * overlap_merge.hpp:158-179; relocalisation; offline re-registration): lio_ndt_align_batch takes the scans as they leave here.  Waits for the
 * result; n_ds[i] (may be NULL) = points of scan i.  Per scan identical to lio_scan_voxel_downsample */
int lio_scan_voxel_downsample_batch(lio_scan** scans, int n, float leaf, uint32_t* n_ds);
/* bypass the filter: use these points as feats_down_body (tests, staged pipelines) */
int lio_scan_set_ds(lio_scan*, const float* ds_body_xyzi, uint32_t n_ds);
int lio_scan_num_ds(lio_scan*);                                                   /* syncs the stream */
int lio_scan_download_ds(lio_scan*, float* out_xyzi, uint32_t cap);              /* feats_down_body */
int lio_scan_download_world(lio_scan*, float* out_xyzi, uint32_t cap);           /* feats_down_world */
/* ABI 19: the downsampled cloud where it lies in HBM (n_ds float4 x y z intensity) and its size; waits for the scan's stream.  NULL when there
 * is none.  The pointer is the scan's own buffer: valid until the scan is written again. */
const void* lio_scan_ds_device(lio_scan*, uint32_t* n);
/* per-point results of the last linearize: any pointer may be NULL.
 * selected[n_ds] (point_selected_surf), normvec[n_ds*4] (n, pd2), nn_cnt[n_ds], nn_pts[n_ds*5*4] */
int lio_scan_download_match(lio_scan*, uint8_t* selected, float* normvec, int32_t* nn_cnt, float* nn_pts);

/* live per-kernel timing with HIP events recorded on the handle's stream around every launch of the three
 * per-pass kernels (bench.py's roofline leg).  Off by default; costs two event records per launch when on. */
typedef struct lio_kernel_times {
    double knn_us, linearize_us, finalize_us;          /* summed device time */
    uint32_t knn_launches, linearize_launches, finalize_launches;
    uint32_t pad;
} lio_kernel_times;
/* on = bit mask of the kernel classes to time: 1 kNN (what bench.py's timed region uses: two event records per
 * kNN launch), 2 linearize (+ report), 0 = off */
int lio_scan_enable_kernel_timing(lio_scan*, int on);
int lio_scan_kernel_times(lio_scan*, lio_kernel_times* out, int reset);

/* normal equations of one pass, all f64, reduced in a fixed order (run-to-run identical) */
typedef struct lio_normal_eq {
    double JtJ[36];      /* sum row6 row6^T, row6 = [n, (R_il p + t_il) x (R_wi^T n)]  (src/laserMapping.cpp:909-931) */
    double Jtr[6];       /* sum row6 * (-pd2)                                               */
    double nnT[9];       /* sum n n^T  (HTH of src/laserMapping.cpp:937)                     */
    double eigvec[9];    /* eigenvectors of nnT as columns, ascending eigenvalue (row-major 3x3) */
    double eigval[3];
    double contri[3];    /* per eigenvector: sum |n^.v| over rows with |n^.v| > 0.1736 (src/laserMapping.cpp:946-964); +inf when
                            the bound eigval[i] - 0.1736^2 n_eff >= 250 already proves "not degenerate" and the pass was skipped */
    double strong[3];    /* ... > 0.7070 */
    double sum_abs_res;  /* total_residual (src/laserMapping.cpp:884) */
    uint32_t n_eff;      /* effct_feat_num */
    uint32_t n_ds;       /* feats_down_size */
    uint32_t n_knn_candidates_lo, n_knn_candidates_hi; /* 64-bit count of in-stencil points visited (kNN passes) */
    uint32_t n_tie;      /* kNN queries redone with the exact (d2, x, y, z) comparison because of an exact d2 tie */
    uint32_t seq;        /* sequence number of this record (the host-side wait spins on it) */
} lio_normal_eq;

/* One evaluation of h_share_model_geometric (src/laserMapping.cpp:813-932) without the host-side
 * degeneracy projection: body->world transform, [redo_knn: stencil kNN into the neighbour cache],
 * esti_plane (include/common_lib.h:236-268), residual gate, and the f64 accumulation of the
 * 6-column Jacobian blocks.  pose_wi = (t_wi[3], q_wi[4]);  ext_il = (t_il[3], q_il[4]). */
int lio_p2plane_linearize(lio_map*, lio_scan*, const double pose_wi[7], const double ext_il[7], int redo_knn,
                          lio_normal_eq* out);
/* how lio_p2plane_linearize treats the degeneracy sums: 0 = auto (evaluated only when the eigenvalue bound does not
 * decide, default), 1 = always, 2 = never (the caller evaluates them itself, e.g. after a cross-GPU reduction) */
int lio_scan_set_degeneracy_mode(lio_scan*, int mode);
/* the degeneracy sums of the last linearize against the given eigenvectors (columns of a row-major 3x3) */
int lio_p2plane_degeneracy(lio_scan*, const double V[9], double contri[3], double strong[3]);
/* rows of the last linearize for the (rare) N_eff < 23 branch of the filter
 * (esekfom.hpp:1715-1744): h_x[n_eff*6] (first six columns) and h[n_eff], selected points in index order */
int lio_p2plane_rows(lio_scan*, const double pose_wi[7], const double ext_il[7], double* h_x6, double* h, uint32_t cap_rows);
/* map_incremental (src/laserMapping.cpp:523-576) with the final state: world transform, need_add test
 * against the cached neighbours, insert.  Returns the number of points inserted. */
int lio_map_incremental(lio_map*, lio_scan*, const double pose_wi[7], const double ext_il[7], float map_leaf,
                        int ekf_inited, double travel);
/* first-scan seeding (src/laserMapping.cpp:1227-1238): insert every downsampled point */
int lio_map_seed(lio_map*, lio_scan*, const double pose_wi[7], const double ext_il[7], double travel);

/* ---------------------------------------------------------------------------------------------
 * Engine: replaces the part of fastlio_main() that follows p_imu->Process
 * (src/laserMapping.cpp:1189-1304) together with esekf::update_iterated_dyn_share_modified
 * (include/IKFoM_toolkit/esekfom/esekfom.hpp:1619-1931) and the constants of fastlio_init
 * (src/laserMapping.cpp:1025-1124).  Host C++ (filter algebra, 23 DoF) over the calls above.
 * State vector (26 doubles): pos3 rot4 R_il4 t_il3 vel3 bg3 ba3 grav3  (use-ikfom.hpp:12-21).
 * ------------------------------------------------------------------------------------------- */
lio_engine* lio_engine_create(int device, float resolution, int stencil, uint64_t max_points, uint64_t max_voxels,
                              uint32_t max_raw, uint32_t max_ds);
/* an engine (state + covariance + scan buffers + stream) that registers scans against a map owned by someone
 * else.  Several such engines may run concurrently from different host threads on one map: the map is then
 * read-only (static-map mode is forced; map_incremental is skipped).  Destroying the engine leaves the map. */
lio_engine* lio_engine_create_shared(lio_map* shared_map, uint32_t max_raw, uint32_t max_ds);
void lio_engine_destroy(lio_engine*);
lio_map* lio_engine_map(lio_engine*);
lio_scan* lio_engine_scan(lio_engine*);
int lio_engine_set_state(lio_engine*, const double s26[26]);
int lio_engine_get_state(lio_engine*, double s26[26]);
int lio_engine_set_cov(lio_engine*, const double P[529]);
int lio_engine_get_cov(lio_engine*, double P[529]);
/* flg_EKF_inited, flg_first_scan, travel_distance, first_lidar_time (src/laserMapping.cpp:97-121) */
int lio_engine_set_flags(lio_engine*, int ekf_inited, int first_scan, double travel, double first_lidar_time);
double lio_engine_travel(lio_engine*);
int lio_engine_is_degenerate(lio_engine*);
/* kf.update_iterated_dyn_share_modified(LASER_POINT_COV) on the scan's current ds points; returns #passes */
int lio_engine_update(lio_engine*);
typedef struct lio_pass_log {
    int32_t knn, n_eff, valid, degenerate;
    double sum_abs_res;
    double JtJ[36]; /* after the degeneracy projection, as consumed by the filter */
    double Jtr[6];
    double dx[23];
} lio_pass_log;
int lio_engine_pass_log(lio_engine*, int i, lio_pass_log* out);
/* the per-scan body of fastlio_main: returns 0 first-scan latch, 1 map seeded, 2 too few points,
 * 3 state updated + map_incremental ENQUEUED, < 0 error.  The insert chain (map_incremental's AddPoints + the LRU list) runs on the map's
 * own stream and is not waited for: the call returns when the state is final, the next scan's upload / motion compensation / downsample
 * run beside it, and whatever reads the map next (the next neighbour search, any lio_map_* call) is ordered behind it.  A map that
 * overflowed (LIO_E_CAPACITY) is therefore reported later, ONCE, by whichever call looks first: the next lio_engine_process_scan /
 * lio_fastlio_main (before it launches anything of its own scan; lio_last_error says the failure is the previous scan's),
 * lio_engine_timings, or lio_engine_flush -- call lio_engine_flush after the last scan of a run, or the last insert's outcome is never seen.
 * With lio_engine_enable_timing(1) the insert is waited for (its time is one of the stage timings). */
int lio_engine_process_scan(lio_engine*, const float* raw_body_xyzi, uint32_t n_raw, double lidar_beg_time);
int lio_engine_process_scan_device(lio_engine*, const void* d_raw_body_xyzi, uint32_t n_raw, double lidar_beg_time);
/* per-stage device time of the last process_scan in microseconds (hipEvent based; the reference's
 * equivalent timers are commented out at src/laserMapping.cpp:1314-1342) */
typedef struct lio_timings {
    float downsample_us, knn_us, linearize_us, insert_us, total_device_us;
    float host_solve_us, total_wall_us;
    int32_t n_knn_pass, n_pass, n_ds, n_eff_last;
    int32_t n_added; /* points map_incremental added; -1 while the scan's insert is still running (see above; lio_engine_flush waits for it) */
    uint64_t knn_candidates; /* in-stencil points visited over all kNN passes (C-bar * N_ds * n_knn) */
    float undistort_us;      /* lio_fastlio_main only: pose upload + point filter + motion compensation kernels */
    float imu_host_us;       /* lio_fastlio_main only: host forward propagation (esekf::predict per IMU sample) */
} lio_timings;
int lio_engine_timings(lio_engine*, lio_timings* out);
int lio_engine_enable_timing(lio_engine*, int on);
/* waits for the map_incremental the last lio_engine_process_scan / lio_fastlio_main enqueued and returns its outcome (LIO_OK, LIO_E_CAPACITY
 * when the map overflowed, LIO_E_DEVICE); nothing pending: LIO_OK.  The reference inserts synchronously inside fastlio_main
 * (laserMapping.cpp:1304): this is where the deferred half of that call ends. */
int lio_engine_flush(lio_engine*);
/* ---------------------------------------------------------------------------------------------------------------
 * The IMU front half: the reference's FastLIO entry points, one to one.  After lio_fastlio_init the engine is driven
 * exactly like the reference's module: sensor threads enqueue, the LIO thread calls lio_fastlio_main in a loop
 * (slam/mapping/fastlio/src/fastlio.cpp:185-210,262-276).
 *   lio_fastlio_init ............ fastlio_init          src/laserMapping.cpp:1025-1124 (extR row-major 3x3); also turns on the
 *                                 map's LRU list with the reference's 100000 voxels / 100 m when the engine owns an empty
 *                                 map created with max_voxels > 100000
 *   lio_fastlio_is_init ......... fastlio_is_init       src/laserMapping.cpp:740-743
 *   lio_fastlio_imu_enqueue ..... fastlio_imu_enqueue   src/laserMapping.cpp:397-415 (acc in m/s^2, divided by 9.81 inside)
 *   lio_fastlio_ins_enqueue ..... fastlio_ins_enqueue   src/laserMapping.cpp:417-441
 *   lio_fastlio_pcl_enqueue ..... fastlio_pcl_enqueue   src/laserMapping.cpp:311-330 + Preprocess::velodyne_handler
 *                                 src/preprocess.cpp:395-451: xyzi float4 + PointAttr::stamp (us relative to the header
 *                                 stamp, common/mapping_types.h:26-29); header_stamp in seconds
 *   lio_fastlio_main ............ fastlio_main          src/laserMapping.cpp:1126-1310: sync_packages (:445-520),
 *                                 ImuProcess::Process (src/IMU_Processing.hpp:408-450: IMU_init :164-236, UndistortPcl
 *                                 :238-406 with esekf::predict esekfom.hpp:279-383), then the scan-matching path
 *   lio_fastlio_odometry ........ fastlio_odometry      src/laserMapping.cpp:692-712 (two row-major 4x4)
 *   lio_fastlio_state ........... fastlio_state         src/laserMapping.cpp:714-738 (20 doubles)
 * lio_fastlio_main returns one of LIO_MAIN_* (the reference returns false for IDLE and true otherwise) or a negative
 * error.  The enqueue calls may come from other threads than lio_fastlio_main (the reference's mtx_buffer). */
#define LIO_MAIN_FIRST_SCAN 0 /* first scan only latches first_lidar_time */
#define LIO_MAIN_SEEDED 1     /* map was empty: seeded with this scan */
#define LIO_MAIN_SKIPPED 2    /* too few points */
#define LIO_MAIN_UPDATED 3    /* state updated, map extended */
#define LIO_MAIN_IMU_INIT 4   /* IMU initialisation still collecting samples (no cloud registered) */
#define LIO_MAIN_IDLE 5       /* sync_packages found nothing to do */
int lio_fastlio_init(lio_engine*, const double extT[3], const double extR[9], int filter_num, int max_point_num, double scan_period,
                     int undistort);
int lio_fastlio_is_init(lio_engine*);
int lio_fastlio_imu_enqueue(lio_engine*, double stamp, const double gyr[3], const double acc_ms2[3]);
/* Where the iterate loop of lio_engine_update / lio_engine_process_scan / lio_fastlio_main runs.  0 (default): on the host -- one
 * device linearisation and one hand-over per pass (esekfom.hpp:1619-1931 driven from the CPU, 8 us of host algebra per pass).  1: on the
 * device (the batched engine's loop for this one scan: one submission, one wait; the calling thread is free meanwhile, the scan takes
 * ~15 % longer).  Results identical (tests/test_gpu_parity.py).  Environment LIO_DEVICE_LOOP=1 sets the default of new engines. */
int lio_engine_set_device_loop(lio_engine*, int on);

/* fastlio_ins_enqueue (src/laserMapping.cpp:417-441) after the ENU -> ego -> IMU rotation the reference applies there:
 * vel_imu = Lidar_R_wrt_IMU * Tve^-1 * (Ve, Vn, Vu), third component zeroed by the caller as :436 does.  Only IMU
 * initialisation reads it (IMU_Processing.hpp:201-204; the wheel-speed rows are compiled out, wheelspeed_en == false) */
int lio_fastlio_ins_enqueue(lio_engine*, double stamp, const double vel_imu[3]);
/* wheelspeed_en (src/laserMapping.cpp:83, a constant false in the reference: its binaries never take the branch).  When enabled, a scan
 * whose last INS sample (lio_fastlio_ins_enqueue) is within 10 ms of the scan's end gets the three velocity rows of
 * h_share_model_wheelspeed (:794-811) appended to its point-to-plane rows in every pass of the update (:994-1012: weight 1e-4, 1e-3 when
 * degenerate, times the rows before them).  Such updates run the iterate loop from the host. */
int lio_fastlio_set_wheelspeed(lio_engine*, int enable);
int lio_fastlio_pcl_enqueue(lio_engine*, const float* xyzi, const uint32_t* stamp_us, uint32_t n, double header_stamp);
/* the same without an intermediate copy (boundary marshalling, numpy_to_pointcloud + preprocessPoints of the reference: slam/src/py_utils.cpp:
 * 149-181, slam/common/slam_base.h:83-85): _stage hands out the pinned staging buffers of the next scan (room for n points), the caller writes
 * the points (already in the INS frame) and stamps straight into them, _commit starts their trip to the device and queues the scan.  One scan
 * staged at a time; the pointers are dead after _commit. */
int lio_fastlio_pcl_stage(lio_engine*, uint32_t n, float** xyzi, uint32_t** stamp_us);
int lio_fastlio_pcl_commit(lio_engine*, uint32_t n, double header_stamp);
/* device-resident scan: the two buffers must stay valid until the lio_fastlio_main call that consumes them returned */
int lio_fastlio_pcl_enqueue_device(lio_engine*, const void* d_xyzi, const void* d_stamp_us, uint32_t n, double header_stamp);
int lio_fastlio_main(lio_engine*);
int lio_fastlio_odometry(lio_engine*, double odom_s[16], double odom_e[16]);
int lio_fastlio_state(lio_engine*, double out[20]);
/* test visibility: p_imu->start_state_point as a 26-double state, feats_undistort (dropped points are NaN), and one
 * esekf::predict step on the host (esekfom.hpp:279-383; Q = diagonal of the 12 x 12 process noise: ng, na, nbg, nba;
 * acc in m/s^2); and one update_iterated_dyn_share_modified (esekfom.hpp:1619-1931) on the host with a caller-supplied
 * measurement model fn(ctx, state26, converge, &n, rows6 n x 6, h n, cap) -> valid, for pinning the filter algebra */
int lio_fastlio_start_state(lio_engine*, double s26[26]);
int lio_fastlio_download_undistorted(lio_engine*, float* out_xyzi, uint32_t cap, uint32_t* n);
typedef int (*lio_meas_fn)(void* ctx, const double* s26, int converge, int* n, double* rows6, double* h, int cap);
int lio_eskf_update_cb(const double s26[26], const double P[529], double R, int max_iter, lio_meas_fn fn, void* ctx, int cap, double s26_out[26],
                       double P_out[529]);
/* ... with the wheel-speed rows (src/laserMapping.cpp:794-811, 994-1012) appended to the model's rows in every pass: ins_vel = the INS velocity in
 * the IMU frame (NULL: none), degenerate = the is_degenerate flag the weight depends on */
int lio_eskf_update_ws_cb(const double s26[26], const double P[529], double R, int max_iter, lio_meas_fn fn, void* ctx, int cap, const double* ins_vel,
                          int degenerate, double s26_out[26], double P_out[529]);
int lio_state_predict(const double s26[26], const double P[529], double dt, const double Q[12], const double acc[3], const double gyro[3],
                      double s26_out[26], double P_out[529]);
/* test visibility, host-only: the DEVICE-resident form of update_iterated_dyn_share_modified (csrc/eskf_dev.h: the filter pass as
 * data-parallel phases, one workgroup per scan on the GPU; here the same source compiled for the host) driven by caller-supplied sums:
 *   fn(ctx, state26, converge, acc29) -> valid: acc29 = the 21 upper-triangle entries of J^T J row by row, 6 of J^T h, sum |r|, N_eff
 *   dfn(ctx, V, cs): the six degeneracy sums (contri[3], strong[3]) against the eigenvectors V (columns of a row-major 3 x 3); called
 *                    only when the eigenvalue bound does not decide
 * Returns the number of pass logs written (<= cap_logs); *status = 1 finished, 2 a pass saw N_eff < 23 (the dense branch of
 * esekfom.hpp:1715-1744 runs on the host: the state is the one BEFORE that pass). */
typedef int (*lio_sums_fn)(void* ctx, const double* s26, int converge, double* acc29);
typedef void (*lio_degeneracy_fn)(void* ctx, const double* V9, double* cs6);
int lio_eskf_update_sums_cb(const double s26[26], const double P[529], double R, int max_iter, int degenerate_detect_en, lio_sums_fn fn,
                            lio_degeneracy_fn dfn, void* ctx, double s26_out[26], double P_out[529], lio_pass_log* logs, int cap_logs, int* status);

/* Joint registration across GPUs (BASELINE.json config 5: sub-maps one per GPU, all-gather of the per-shard
 * J^T J / J^T r sums).  When a hook is set the engine calls it after every device linearisation with its LOCAL sums and
 * continues with whatever the hook leaves in the buffer (the GLOBAL sums, identical on every rank):
 *   first call,  n = 29: buf[0..20] J^T J upper triangle (row-major), buf[21..26] J^T r, buf[27] sum|r|, buf[28] n_eff
 *   second call, n = 6 (only when the degeneracy bound on the GLOBAL eigenvalues does not decide): contri[3], strong[3]
 * Every rank then runs the same 23-DoF update on the same numbers.  With a hook the N_eff < 23 branch of the filter
 * uses the information form (rows live on different GPUs). */
typedef void (*lio_reduce_fn)(void* ctx, double* buf, int n);
int lio_engine_set_reduce_hook(lio_engine*, lio_reduce_fn fn, void* ctx);
/* The same natively, over RCCL (librccl = the ROCm build of NCCL; xGMI between the GPUs of a node), for hosts that are not Python: one process
 * per GPU.  lio_comm_unique_id: rank 0 makes the 128-byte id and ships it to the other ranks by whatever the application has (MPI, a socket,
 * torch.distributed's store); lio_comm_init: ncclCommInitRank on `device` (a world of one needs no id and no RCCL).
 * lio_allgather_normal_eq: DEVICE buffers in and out -- every rank contributes one 32-double record (21 J^T J upper triangle, 6 J^T r, sum |r|,
 * N_eff, 3 spare), receives all of them rank-major (world x 32) and, if d_sum32 is given, their sum in fixed rank order (a one-wave kernel:
 * every rank forms the identical bits).  `stream` (a hipStream_t, NULL = the communicator's own) orders it with the caller's kernels.
 * lio_engine_set_joint: joint registration of ONE scan against sub-maps spread over engines and GPUs -- `e` drives the filter; after every
 * linearisation its sums are joined, in this order, by those of the `others` (further sub-maps resident on this GPU, each engine with its own
 * map) and then by the other ranks' through `comm` (NULL = single process).  Replaces a hook set by lio_engine_set_reduce_hook.
 * lio_engine_joint_register: uploads the cloud to every local engine, runs the registration; prior in, posterior out. */
typedef struct lio_comm lio_comm;
int lio_comm_unique_id(uint8_t id[128]);
lio_comm* lio_comm_init(int device, int rank, int world, const uint8_t id[128]);
void lio_comm_destroy(lio_comm*);
int lio_comm_rank(const lio_comm*);
int lio_comm_world(const lio_comm*);
int lio_allgather_normal_eq(lio_comm*, const double* d_local32, double* d_gathered, double* d_sum32, void* stream);
/* the same for the records of many scans at once (the batched engine's joint mode: one collective per pass for all scans of a round):
 * n_records x 32 doubles per rank in, world x n_records x 32 out (rank-major), no sum -- the consumer adds the ranks' records in rank order */
int lio_allgather_records(lio_comm*, const double* d_local, double* d_gathered, uint32_t n_records, void* stream);
int lio_comm_stats(lio_comm*, uint64_t* n_collectives, double* total_us);  /* collectives issued by joint registrations and their host-observed time */
int lio_engine_set_joint(lio_engine* e, lio_engine** others, int n_others, lio_comm* comm);
int lio_engine_joint_register(lio_engine* e, const float* raw_body_xyzi, uint32_t n_raw, double lidar_beg_time, double state26[26], double cov[529]);
int lio_engine_joint_register_device(lio_engine* e, const void* d_raw_body_xyzi, uint32_t n_raw, double lidar_beg_time, double state26[26], double cov[529]);
/* Throughput mode: register a batch of independent scans with `n_engines` engines running concurrently (one host
 * thread + HIP stream per engine, jobs handed out through an atomic counter).  Every job = set_state(state_in) +
 * set_cov(cov_in) + lio_engine_process_scan_device(d_raw, n_raw, lidar_beg_time); outputs are filled per job.
 * Intended for engines created with lio_engine_create_shared on one read-only map (independent scans of several
 * sensors / sequences, relocalisation candidates, map-merge alignments). */
#define LIO_JOB_KEEP_CACHE 1u
#define LIO_JOB_IDLE 2u         /* lio_batch_sequences_step: the session of this job has no scan this round (rc = 0, nothing else is looked at) */
#define LIO_JOB_HOST_RAW 4u     /* lio_batch_process / lio_engines_process_batch: d_raw points to HOST memory (pinned for full PCIe rate: lio_pinned_alloc);
                                   the library copies the cloud to HBM on the round's stream, overlapped with the other rounds in flight -- the copy
                                   the reference's boundary starts with (slam/src/py_utils.cpp:149-181, slam_wrapper.cpp:64-84).  The host buffer must
                                   stay valid and unchanged until the call that took the job returns (the copy is asynchronous).  Not accepted by
                                   lio_batch_sequences_step (rc = LIO_E_INVALID).  Appended in round 5 */
#define LIO_JOB_FLAGS_KNOWN 7u  /* every other bit must be zero: a job with unknown bits is rejected (rc = LIO_E_INVALID), so that an uninitialised
                                   word cannot silently pick a behaviour */
typedef struct lio_scan_job {
    const void* d_raw;          /* device pointer, XYZI float4 */
    uint32_t n_raw;
    uint32_t flags;             /* ABI note: until round 3 this word was padding and ignored.  ZERO-INITIALISE the job array (memset / = {0}).
                                   0 (default): the jobs are INDEPENDENT scans -- the engine / slot that takes the job first forgets its neighbour
                                   cache, as fastlio_init does for Nearest_Points (src/laserMapping.cpp:1045-1047), so the result does not depend
                                   on which scan that engine registered before; LIO_JOB_KEEP_CACHE: a job of a sequence -- the cache of the
                                   previous scan survives (Nearest_Points across fastlio_main calls, stale where a search finds nothing): callers that
                                   feed CONSECUTIVE scans of one sensor through a batch API and want fastlio_main's carry-over must set it */
    double lidar_beg_time;
    const double* state_in;     /* 26 doubles */
    const double* cov_in;       /* 529 doubles */
    double* state_out;          /* 26 doubles, may be NULL */
    int32_t rc;                 /* return code of process_scan */
    int32_t n_ds, n_pass, n_knn_pass;
} lio_scan_job;
int lio_engines_process_batch(lio_engine** engines, int n_engines, lio_scan_job* jobs, int n_jobs);
/* Throughput mode, batched: B scans per launch.  A batch owns `n_groups` groups of `n_slots` slots (scan buffers + a device-resident
 * filter each); lio_batch_process hands the jobs to the groups round-robin from ONE host thread: a round = one small upload (states,
 * covariances, descriptors), the voxel-grid chain and (maximum_iter + 1) x {stencil kNN where the filter asks for it, linearisation,
 * filter pass} enqueued blind on the group's stream -- every launch serves all slots (blockIdx.y = slot), the iterate loop of
 * update_iterated_dyn_share_modified (esekfom.hpp:1619-1931) runs on the device (csrc/eskf_dev.h), and the host sees one result record per
 * scan in mapped memory.  Same job semantics and results as lio_engines_process_batch on engines created with lio_engine_create_shared
 * (static map: map_incremental is skipped); a pass that needs the N_eff < 23 dense branch of the filter is finished on the host. */
typedef struct lio_batch lio_batch;
typedef struct lio_batch_result {
    double state[26];
    int32_t status;        /* 1 finished on the device, 2 a pass saw 1 <= N_eff < 23: state / loop_* are those BEFORE that pass */
    int32_t n_pass, n_knn_pass, n_ds, n_eff, degenerate, radix_passes, err;
    int32_t loop_i, loop_t, loop_converge, pad;
    uint32_t seq, pad2;
} lio_batch_result;
lio_batch* lio_batch_create(lio_map* shared_map, int n_slots, int n_groups, uint32_t max_raw, uint32_t max_ds);
/* Joint registration, batched (BASELINE.json config 5, the map-merge shape of slam/localization/include/overlap_merge.hpp:46-48,158-179: many key
 * frames x candidates, each an independent alignment): every job of lio_batch_process is registered against ALL `sub_maps` (resident on this GPU)
 * and, through `comm` (NULL: single process), against the sub-maps of the other ranks -- every rank calls lio_batch_process with the SAME job list
 * (same clouds resident on its own GPU, same priors) and receives the same posteriors, bit for bit.  A round of B scans is enqueued blind on the
 * round's stream: downsample once per scan, then per pass {neighbour search, linearisation} per local sub-map, the rank's B records of 32 doubles,
 * ONE all-gather of [B x 32] doubles for the whole round (RCCL on that stream, no host in between), the filter pass on the sums taken in rank
 * order (csrc/eskf_dev.h on the device).  A pass with N_eff < 23 uses the information form (the rows live on several GPUs), a scan whose pass needs
 * the degeneracy sums (src/laserMapping.cpp:946-964) is redone by the host-driven path (lio_engine_joint_register_device of the slot's engines).
 * Results equal lio_engine_joint_register's on the same sub-maps, job by job (tests/test_dist.py). */
lio_batch* lio_batch_create_joint(lio_map** sub_maps, int n_sub_maps, lio_comm* comm, int n_slots, int n_groups, uint32_t max_raw, uint32_t max_ds);
/* the collective of the joint mode through a caller-supplied function instead of RCCL (embedding in a host that has its own transport; and the
 * way the world > 1 logic is exercised where RCCL cannot be -- two ranks on ONE GPU over gloo, tests/test_dist.py): called on the submitting
 * thread once per round and pass with this rank's [n_records x 32] doubles in device memory, it must leave every rank's records, rank-major
 * ([rank][record][32]), in d_gathered before it returns (work already enqueued on `stream` precedes the call; what follows is enqueued after).
 * For a batch created by lio_batch_create_joint WITHOUT a communicator; a scan that needs the host-driven path (degeneracy sums) fails with
 * LIO_E_STATE in this mode. */
typedef int (*lio_gather_fn)(void* ctx, const double* d_local, double* d_gathered, uint32_t n_records, void* stream);
int lio_batch_set_gather_hook(lio_batch*, lio_gather_fn fn, void* ctx, int rank, int world);
/* With more than one rank a joint round's voxel-grid chain (src/laserMapping.cpp:1206-1208, once per scan) runs on ONE rank per scan -- rank r owns the
 * slots [r * ceil(B / world), ...) -- and the downsampled clouds reach the others in one all-gather per round of fixed-size slot chunks (the same
 * transport as the records; with a hook, n_records = chunk bytes / 256).  The chunk holds 1.25 x the largest cloud the batch has registered so far
 * (derived from the results, hence equal on every rank); a cloud that does not fit voids the round's result for that job on every rank and the job runs
 * again with full-size chunks.  LIO_JOINT_SPLIT_DS=0 in the environment: every rank downsamples every scan, as up to ABI revision 5 (bit-identical
 * results either way: tests/test_dist.py).  Statistics: points per chunk now in force (0 before the first round), jobs that ran again, bytes one rank
 * contributes to a round's all-gather. */
int lio_batch_exchange_stats(lio_batch*, uint32_t* chunk_points, uint64_t* jobs_rerun, uint64_t* bytes_per_rank_and_round);
/* Sequence mode: throughput WITH map_incremental.  n_groups x n_slots independent SLAM sessions (replay of recorded drives, offline mapping of many
 * sequences), one per slot, each with ITS OWN map (lio_engine_create's arguments, per session).  lio_batch_sequences_step takes exactly one job per
 * session -- job j is the NEXT scan of session j = (group j / n_slots, slot j % n_slots): state_in / cov_in the propagated prior as for every
 * lio_scan_job, LIO_JOB_IDLE for a session without a scan this round -- and runs, per group, fastlio_main from the downsample to map_incremental
 * (src/laserMapping.cpp:1193-1304) as ONE blind submission: voxel-grid chain, (maximum_iter + 1) x {stencil kNN against the slot's own map,
 * linearisation, filter pass on the device}, then for every slot whose update finished classify + IVox::AddPoints (+ the LRU list) -- every launch
 * serves all slots (blockIdx.y = slot).  SURVEY 8d's B_ins, which the static batch leaves out, is inside the round.  The file-scope state of
 * laserMapping.cpp (first_lidar_time, flg_EKF_inited, travel, the stencil switch at 10 x INIT_TIME) lives in the slot's engine
 * (lio_batch_engine(b, group, slot); its map: lio_engine_map).  Scans a round cannot take go through that engine's own code -- a session's first
 * scan (only its time is kept, rc 0) and its map seed (rc 1), a scan whose pass needs the dense N_eff < 23 branch, a bounding box that needs more
 * radix passes than were launched -- so a session driven here and the same scans pushed one by one through lio_engine_set_state / set_cov /
 * lio_engine_process_scan_device on an engine with lio_engine_set_device_loop(e, 1) give the same bits (tests/test_sequence_batch_gpu.py).
 * rc per job as lio_engine_process_scan; state_out and cov_out[j * 529 ..] (may be NULL) receive the posterior (the prior where nothing was
 * registered).  The pass logs of a scan registered inside a round stay on the device (lio_engine_pass_log of the slot's engine is empty).
 * A step that returns a device error after some of its groups' rounds already ran leaves those sessions' maps one sweep ahead of their engines: the
 * batch then refuses further steps (LIO_E_STATE) -- destroy it; a step that fails before any round ran can be repeated. */
lio_batch* lio_batch_create_sequences(int device, float resolution, int stencil, uint64_t max_points, uint64_t max_voxels, int n_slots, int n_groups,
                                      uint32_t max_raw, uint32_t max_ds);
int lio_batch_sequences_step(lio_batch*, lio_scan_job* jobs, int n_jobs, double* cov_out);
/* lio_fastlio_main (= fastlio_main, src/laserMapping.cpp:1160-1310) for every session of a sequence batch at once: replay of many recorded drives
 * through the reference's own entry points.  Each session's engine carries the front half -- lio_fastlio_init(lio_batch_engine(b, g, s), ...), then
 * lio_fastlio_imu_enqueue / lio_fastlio_ins_enqueue / lio_fastlio_pcl_enqueue[_device] on it as for a single engine.  One call = one fastlio_main per
 * session: sync_packages, IMU initialisation, forward propagation and undistortion per session as lio_fastlio_main does them, ONE sequence round for
 * the scans that reach registration, the back half per session.  rc_out[j] (n_groups x n_slots entries) = what lio_fastlio_main would have returned
 * for session j (LIO_MAIN_IDLE without a complete package); lio_fastlio_odometry / _state of the session's engine read the result.  Same bits as
 * lio_fastlio_main on a per-session engine with the device loop on (tests/test_sequence_batch_gpu.py). */
int lio_batch_fastlio_main(lio_batch*, int* rc_out);
void lio_batch_destroy(lio_batch*);
int lio_batch_process(lio_batch*, lio_scan_job* jobs, int n_jobs);
/* live kernel timing of the batched chain with HIP events on the groups' streams (bench.py's roofline leg): per class the summed device
 * time and the number of timed launches (a "downsample" launch = the whole voxel-grid chain of one round; a kNN / linearise / filter-pass
 * launch = one kernel serving all slots of a round).  Off by default. */
typedef struct lio_batch_times {
    double downsample_us, knn_us, linearize_us, step_us;
    uint32_t downsample_launches, knn_launches, linearize_launches, step_launches;
    double insert_us;            /* sequence mode: the map_incremental half of a round (classify + AddPoints + LRU + read-back records); appended in round 4 */
    uint32_t insert_launches, pad;
} lio_batch_times;
/* on: 0 off, 1 timing, 2 (or 3) timing with the counting variant of the kNN kernel (lio_map_knn_touched) -- times of that variant are not
 * the product's */
int lio_batch_enable_kernel_timing(lio_batch*, int on);
int lio_batch_kernel_times(lio_batch*, lio_batch_times* out, int reset);
/* test visibility: the engine behind slot `slot` of group `group` (its scan buffers, pass log of a host continuation) */
lio_engine* lio_batch_engine(lio_batch*, int group, int slot);
/* on: process_scan skips map_incremental -- scan-to-map registration against a prebuilt static map
 * (BASELINE.json configs 2 and 4); off (default): the reference's mapping behaviour */
int lio_engine_set_static_map(lio_engine*, int on);

/* ---------------------------------------------------------------------------------------------
 * Localization matcher: replaces fast_gicp::NDTCuda<PointXYZI, PointXYZI> as select_registration_method("NDT_CUDA")
 * configures it (slam/backend/hdl_graph_slam/src/hdl_graph_slam/registrations.cpp:105-118: P2D, resolution 1.0,
 * DIRECT7) behind pcl::Registration's setInputTarget / setInputSource / align
 * (slam/localization/hdl_localization/src/hdl_localization/pose_estimator.cpp:246-247).
 * The source cloud is a lio_scan (upload + lio_scan_voxel_downsample with leaf = map_resolution, as
 * hdl_localization_nodelet.cpp:333-344 does); transforms are row-major 4x4 doubles.
 * ------------------------------------------------------------------------------------------- */
typedef struct lio_ndt lio_ndt;
/* NDTCuda() + setResolution + setNeighborSearchMethod(DIRECT1 / DIRECT7 / DIRECT27  ->  search_method 1 / 7 / 27) */
lio_ndt* lio_ndt_create(int device, float resolution, int search_method, uint64_t max_points, uint64_t max_voxels, uint32_t max_source_points);
void lio_ndt_destroy(lio_ndt*);
/* setInputTarget -> NDTCudaCore::set_target_cloud -> create_target_voxelmap (ndt_cuda.cu:105-141): Gaussian voxel map
 * (mean, covariance), PLANE regularisation, inverse covariance.  Replaces any previous target. */
int lio_ndt_set_target(lio_ndt*, const float* xyzi, uint64_t n);
int lio_ndt_set_target_device(lio_ndt*, const void* d_xyzi, uint64_t n);
int lio_ndt_num_voxels(lio_ndt*);
/* diagnostic: statistics of the voxel that contains p; returns its point count (0 = no such voxel) */
int lio_ndt_voxel_at(lio_ndt*, const float p[3], float mean[3], float cinv[9]);
/* NDTCuda::linearize (update_corr = 1, with_derivatives = 1: update_correspondences + compute_error with H, b) and
 * NDTCuda::compute_error (update_corr = 0, with_derivatives = 0: error on the cached pairs)  (ndt_cuda_impl.hpp:82-90) */
int lio_ndt_linearize(lio_ndt*, lio_scan* source, const double T[16], int update_corr, int with_derivatives, double H[36], double b[6],
                      double* err, uint32_t* n_corr);
/* pcl::Registration::getFitnessScore(max_range) as pose_estimator.cpp:262 calls it (max_range 25 = a SQUARED distance): mean
 * squared distance from the transformed source points to their nearest target point, over those within range; *score is
 * DBL_MAX when none is (PCL's value).  Exact nearest neighbours, from the target points the voxel grid retains. */
int lio_ndt_fitness_score(lio_ndt*, lio_scan* source, const double T[16], double max_range, double* score, uint32_t* n_inliers);
/* calc_fitness_score(cloud1, cloud2, relpose, max_range) of the map-merge / loop-closure tools, slam/localization/include/overlap_merge.hpp:
 * 206-263: the target is cloud1 after `filter` (:196-204: sqrt(x^2 + y^2) < xy_range && z > min_z -- applied by the caller before
 * lio_ndt_set_target), the source is cloud2 (all its points: lio_scan_set_ds), transformed by relpose (pcl::transformPointCloud, f32) and
 * then put through the same filter here.  *score = mean squared nearest-neighbour distance over the source points whose neighbour is
 * within max_range (squared, as PCL's kd-tree returns it), *inlier_ratio = their share of the filtered source; (DBL_MAX, 0) if none.
 * The reference's constants: xy_range 100.0, min_z 0.5. */
int lio_ndt_overlap_score(lio_ndt*, lio_scan* source, const double relpose[16], double max_range, double xy_range, double min_z, double* score,
                          double* inlier_ratio);
/* live timing of the matcher's dominant kernel (ndt_cost_kernel: correspondences + cost [+ H, b] of one evaluation) with HIP events on the
 * stream it runs on -- bench.py's roofline leg of BASELINE config 4.  Summed over the evaluations since the last reset: device time, launches
 * (of which with a correspondence update), voxel correspondences evaluated, source points.  Off by default (one event wait per evaluation). */
typedef struct lio_ndt_times {
    double cost_us;
    uint64_t launches, update_launches, pairs, source_points;
} lio_ndt_times;
int lio_ndt_enable_kernel_timing(lio_ndt*, int on);
int lio_ndt_kernel_times(lio_ndt*, lio_ndt_times* out, int reset);
typedef struct lio_ndt_params {
    int32_t max_iterations;           /* setMaximumIterations (64) */
    int32_t lm_max_iterations;        /* lm_max_iterations_ (10) */
    double rotation_epsilon_deg;      /* setRotationEpsilon (0.1) */
    double transformation_epsilon;    /* setTransformationEpsilon (0.01) */
    double lm_init_lambda_factor;     /* 1e-9 */
    double max_process_time_ms;       /* setMaxProcessTime; <= 0: no wall-clock cut-off */
} lio_ndt_params;
void lio_ndt_default_params(lio_ndt_params*);
/* pcl::Registration::align(guess) -> LsqRegistration::computeTransformation with step_lm
 * (lsq_registration_impl.hpp:71-109,163-208); out = final transformation, *converged = hasConverged().  step_lm's compute_error(xi) and the
 * linearize(xi) that follows an accepted step are fetched in one launch (see lio_ndt_align_batch): identical results, one device hand-over per
 * LM iteration instead of two. */
int lio_ndt_align(lio_ndt*, lio_scan* source, const double guess[16], const lio_ndt_params* params, double out[16], int* iterations,
                  int* converged);

/* Batched alignments: the map-merge / loop-closure / relocalisation tools evaluate several candidates per key frame (slam/localization/include/
 * overlap_merge.hpp:158-179: 64 key frames x <= 3 candidates, every one an independent registration->align) -- here B of them per launch against
 * one or several targets: slot = (target, source scan, guess), the Levenberg-Marquardt loop of LsqRegistration (lsq_registration_impl.hpp:71-208) resident on the
 * device, a round = {cost evaluation of the slots that linearise, of the slots that try a step, LM kernel}, every launch serving all slots; the
 * host looks at the slots' states every six rounds.  A trial evaluation is speculative (round 4): one launch computes the trial's cost on the
 * pairs cached at the linearisation point AND the linearisation at the trial pose, which an accepted step continues from -- one round per LM
 * iteration instead of two, the same numbers (lio_ndt_align does the same, LIO_NDT_SPEC=0 turns it off there).  Same schedule, stopping rules
 * and results as lio_ndt_align job by job (to the rounding of the device's libm); max_process_time_ms does not apply.  `evaluations` counts
 * launches that served the job (1 + the LM trials).  Sources: lio_scan objects holding their downsampled clouds (lio_scan_voxel_downsample /
 * lio_scan_set_ds), at most max_source_points each. */
typedef struct lio_align_job {
    lio_ndt* target;         /* NULL: the matcher the call is made on; else another target of the same resolution / search method / device
                                (a new key frame against each of its candidate frames: setInputTarget per candidate in the reference) */
    lio_scan* source;
    const double* guess;     /* row-major 4 x 4 */
    double out[16];          /* final transformation */
    int32_t iterations, converged, evaluations, rc;
} lio_align_job;
int lio_ndt_align_batch(lio_ndt*, lio_align_job* jobs, int n_jobs, const lio_ndt_params* params);

/* ---------------------------------------------------------------------------------------------
 * Generalized-ICP: replaces fast_gicp::FastGICP<PointXYZI, PointXYZI> as select_registration_method("FAST_GICP") configures it
 * (slam/backend/hdl_graph_slam/src/hdl_graph_slam/registrations.cpp:33-42) -- the fine matcher of the map merge / loop closure tools
 * (slam/localization/include/overlap_merge.hpp:54-58,158-179: coarse NDT -> fine GICP -> fitness) and, through the same cost function, the
 * matcher family of slam/thirdparty/fast_gicp/include/fast_gicp/gicp/impl/{fast_gicp_impl.hpp:118-303, fast_vgicp_impl.hpp:72-204}:
 *   create ......... FastGICP() + setCorrespondenceRandomness(k); grid_resolution = cell size of the search grid (results do not depend on it)
 *   set_target / set_source  setInputTarget / setInputSource: exact k nearest neighbours of every point, covariance, PLANE regularisation
 *   linearize ...... update_correspondences (nearest target point within max_corr_dist, Mahalanobis (C_B + R C_A R^T)^-1) + linearize:
 *                    H = sum J^T M J, b = sum J^T M e, err = sum e^T M e (update_corr = 0: the cached pairs; with_derivatives = 0: compute_error)
 *   align .......... pcl::Registration::align(guess) -> LsqRegistration's LM loop; params NULL = the reference's FAST_GICP settings
 *   download / correspondences  test visibility: the clouds in internal (grid) order with their regularised covariances (xx, xy, xz, yy, yz, zz);
 *                    the target index of every source point (-1 = none), in that order
 *   neighbours / mahalanobis  test visibility, see below
 * Transforms are row-major 4 x 4 doubles.
 * "Exact" means: the neighbour list of point i is the k smallest keys (d2, index), d2 = (ex*ex + ey*ey) + ez*ez in f32 and the index in internal
 * order, so ties of distance and duplicate points are decided; a pair is the smallest such key over the target, taken iff d2 < (float)(max_corr_dist^2)
 * strictly.  Both searches walk rings of grid cells (rings 0 .. 65 for the neighbours, 0 .. 16 for the pairs) and, when that has not settled
 * the answer, go over the whole cloud instead: the result is the same at any distance and any grid_resolution, only the time differs.
 * Input contract: coordinates are finite (set_target / set_source: LIO_E_INVALID otherwise, the object unchanged; the intensity is not read);
 * the pose is finite and max_corr_dist is >= 0, +inf = no limit (linearize / align: LIO_E_INVALID otherwise, nothing launched).  A source point
 * whose TRANSFORMED position overflows f32 gets no pair.  A finite coordinate may be of any size: where |x / grid_resolution| is past 2^21 the
 * cells alias (the key keeps 21 bits per axis: more candidates, the same result), past 2^24 the distance to the cell's face is taken as
 * unknown, and past the int range (or where the quotient overflows f32) the cell index saturates and the search of that point goes over the
 * whole cloud; in all of these the lists and pairs stay the exact ones, only the time differs.  Clouds that enter on the device (the loop detector's and the overlap detector's key
 * frames, which go through the same covariance kernel) are not checked: they are required to hold finite points. */
typedef struct lio_gicp lio_gicp;
lio_gicp* lio_gicp_create(int device, float grid_resolution, uint32_t max_points, int k_correspondences);
void lio_gicp_destroy(lio_gicp*);
int lio_gicp_set_target(lio_gicp*, const float* xyzi, uint32_t n);
int lio_gicp_set_source(lio_gicp*, const float* xyzi, uint32_t n);
/* ABI 19: the same two calls for a cloud that lies in HBM (n float4 x y z intensity, complete: whatever wrote it has been waited for).  The
 * contract is the host entry's: more than max_points is LIO_E_CAPACITY, fewer than k points or a coordinate that is not finite is LIO_E_INVALID
 * (a kernel counts such points and one word comes back), and a refused call leaves the matcher as it was.  The staging copy is device to device;
 * from there on the path is the host entry's (grid, covariance kernel, the source's copy in caller order).  All four entries leave the cloud
 * in ONE internal order, a function of the cloud alone: the grid's cells by the lowest caller row among their points, a cell's points by
 * rising caller row (the grid's own arrival order is put right after the insertion).  So the same points set from either side, on any handle,
 * any number of times, give the same bits in lio_gicp_download, lio_gicp_align and lio_gicp_fitness_score. */
int lio_gicp_set_target_device(lio_gicp*, const void* d_xyzi, uint32_t n);
int lio_gicp_set_source_device(lio_gicp*, const void* d_xyzi, uint32_t n);
/* The voxelised variant, fast_gicp::FastVGICP (fast_vgicp_impl.hpp:72-204; select_registration_method("FAST_VGICP"), registrations.cpp:56-66:
 * the reference's matcher on machines without CUDA): voxel_resolution > 0 turns the target into Gaussian voxels (mean position, mean of the
 * points' regularised 20-NN covariances: ADDITIVE mode, fast_vgicp_voxel.hpp:95-110,129-167) and lio_gicp_linearize / _align into its
 * update_correspondences / linearize / compute_error: a source point corresponds to the voxel its transformed position falls in
 * (search_method 1 = DIRECT1, the reference's default; 7, 27: the neighbours too), weight sqrt(points in the voxel); max_corr_dist is not
 * used.  0 = back to the kd-tree form.  The resolution should be exactly representable in f32 (the reference's 1.0 is). */
int lio_gicp_set_voxel_mode(lio_gicp*, double voxel_resolution, int search_method);
/* diagnostic: the Gaussian voxel of the target holding point p -> number of points (0: none), mean[3], covariance (xx, xy, xz, yy, yz, zz) */
int lio_gicp_voxel_at(lio_gicp*, const float p[3], double mean[3], double cov6[6]);
int lio_gicp_download(lio_gicp*, int which, float* xyzi, double* cov6, uint32_t cap);
int lio_gicp_correspondences(lio_gicp*, int32_t* corr, uint32_t cap);
/* diagnostics (ABI 17).  neighbours: the sorted neighbour list of every point of cloud `which` (0 target, 1 source) as the covariance kernel holds
 * it, idx[i * 32 + j] = internal index of the j-th nearest of point i (point i itself included), ascending (d2, index); places >= k hold further
 * candidates no nearer than the k-th, or -1.  Runs the search again on the cloud's grid; the cloud and its covariances stay as they are.  Returns the
 * number of points; LIO_E_STATE for a cloud without a grid (none set, or a source that was adopted on the device as it stands), LIO_E_CAPACITY for
 * cap_points < n.  mahalanobis: (xx, xy, xz, yy, yz, zz) of (C_B + R C_A R^T)^-1 for every source point as the last linearize with update_corr
 * left it; a row whose correspondence is -1 is undefined.  LIO_E_STATE in voxel mode (its matrices are per (point, voxel) and not exposed). */
int lio_gicp_neighbours(lio_gicp*, int which, int32_t* idx, uint32_t cap_points);
int lio_gicp_mahalanobis(lio_gicp*, double* maha6, uint32_t cap);
int lio_gicp_linearize(lio_gicp*, const double T[16], double max_corr_dist, int update_corr, int with_derivatives, double H[36], double b[6], double* err,
                       uint32_t* n_corr);
int lio_gicp_align(lio_gicp*, const double guess[16], const lio_ndt_params* params, double max_corr_dist, double out[16], int* iterations, int* converged);
/* pcl::Registration::getFitnessScore(max_range) of the handle's pair under T (the loop section's "fitness" rule: the source moved by T cast to
 * f32, the exact nearest target point by the f32 d2, the bound applied to the SQUARED distance, f64 sum / count; DBL_MAX when nr = 0).  The
 * sum runs over the source in the order lio_gicp_set_source was given it, by the loop detector's kernel: for a pair that is also in a lio_loop
 * bank, score and nr are lio_loop_align_candidates'.  nr may be NULL */
int lio_gicp_fitness_score(lio_gicp*, const double T[16], double max_range, double* score, uint32_t* nr);

/* ---------------------------------------------------------------------------------------------------------------
 * The localisation loop around the matcher: hdl_localization::PoseEstimator (slam/localization/hdl_localization/src/
 * pose_estimator.cpp) = a 23-state unscented Kalman filter (include/kkl/alg/unscented_kalman_filter.hpp:42-262 over
 * include/hdl_localization/pose_system.hpp:14-115; f32 like the reference), host C++:
 *   create ........ PoseEstimator::PoseEstimator      pose_estimator.cpp:22-66 (imu_ext row-major 4 x 4, quaternion (w, x, y, z))
 *   predict ....... predict(stamp) / predict(stamp, acc, gyro)   :142-186 (acc, gyro NULL = no IMU); returns 1 if a step was made
 *   match ......... match(observation, ..., stamp, cloud, gps = none, ...)  :188-300: lio_ndt_align from the filter's pose, the
 *                   5 m / 10 deg gate, quaternion hemisphere; returns 1 / 0 = the reference's bool
 *   correct ....... correct(stamp, observation)       :348-360
 *   matrix / get .. matrix(), ukf->mean / cov
 *   guess / observe  the two host halves of match() around the alignment (:196-247 / :250-302), with the GNSS observation fused in
 *                   (fusion_pose :420-433); match_gps = guess -> lio_ndt_align -> observe; match_gps_only = the scan-less match :304-346
 *   get_timed_pose  get_timed_pose + the INS state queue (:104-141), re-predicted by correct (:366-381); predict_nostate :70-86
 * The fitness score of the warm-up phase is lio_ndt_fitness_score.  predict / predict_nostate / get_timed_pose / correct hold the handle's
 * mutex, as the reference's data_mutex does (the INS callback thread against the scan thread); the other calls belong to the scan thread. */
typedef struct lio_pose_estimator lio_pose_estimator;
typedef struct lio_gps_observation {  /* what match() reads of an RTKType: T (map-frame pose, row-major), precision, dimension (2 / 3 / 6) */
    double T[16];
    double precision;
    int32_t dimension;
} lio_gps_observation;
lio_pose_estimator* lio_pose_estimator_create(const float imu_ext[16], uint64_t stamp_us, const float pos[3], const float quat_wxyz[4],
                                              double cool_time_duration);
void lio_pose_estimator_destroy(lio_pose_estimator*);
int lio_pose_estimator_predict(lio_pose_estimator*, uint64_t stamp_us, const float acc[3], const float gyro[3]);
int lio_pose_estimator_match(lio_pose_estimator*, lio_ndt* target, lio_scan* source, const lio_ndt_params* params, float observation[7],
                             int* iterations);
int lio_pose_estimator_match_gps(lio_pose_estimator*, lio_ndt* target, lio_scan* source, const lio_ndt_params* params, const lio_gps_observation* gps,
                                 float observation[7], float observation_cov[49], int* iterations);
int lio_pose_estimator_guess(lio_pose_estimator*, const lio_gps_observation* gps, float init_guess[16]);
int lio_pose_estimator_observe(lio_pose_estimator*, const float init_guess[16], const float aligned[16], int converged, const lio_gps_observation* gps,
                               float observation[7], float observation_cov[49]);
int lio_pose_estimator_match_gps_only(lio_pose_estimator*, const lio_gps_observation* gps, float observation[7], float observation_cov[49]);
int lio_pose_estimator_get_timed_pose(lio_pose_estimator*, uint64_t stamp_us, const double acc_g[3], const double gyro_dps[3], double pose[16]);
int lio_pose_estimator_predict_nostate(lio_pose_estimator*, uint64_t stamp_us, double pose[16]);
int lio_pose_estimator_correct(lio_pose_estimator*, uint64_t stamp_us, const float observation[7]);
uint64_t lio_pose_estimator_get_dt(lio_pose_estimator*);  /* get_dt() :389-391, us */
int lio_pose_estimator_get(lio_pose_estimator*, float mean23[23], float cov529[529]);
int lio_pose_estimator_set(lio_pose_estimator*, const float mean23[23], const float cov529[529]);
int lio_pose_estimator_matrix(lio_pose_estimator*, float T[16]);

/* ---------------------------------------------------------------------------------------------------------------
 * Local-map assembly for localisation on the device: Localization::runUpdateLocalMap (slam/localization/src/
 * localization.cpp:303-373).  Key-frame clouds (map frame) are stored once in HBM; lio_localmap_update does one pass of the
 * loop body -- skip if the pose moved less than update_distance (10 m) since the last update, radius search (30 m) over the
 * key-frame positions nearest first, thinning by key_frame_distance, concatenation until max_local_points (200000), VoxelGrid
 * with `leaf`, new NDT target -- with device-to-device copies only.  Returns 0 nothing to do, 1 target replaced, 2 out of map
 * (:364-367), 3 nearest key frame >= 20 m away (:352-354); the target is dropped in cases 2 and 3. */
typedef struct lio_localmap lio_localmap;
lio_localmap* lio_localmap_create(int device, uint64_t max_total_points, uint32_t max_local_points, uint32_t max_keyframe_points);
void lio_localmap_destroy(lio_localmap*);
int lio_localmap_add_keyframe(lio_localmap*, const float* world_xyzi, uint32_t n, const float position[3]);
int lio_localmap_num_keyframes(lio_localmap*);
int lio_localmap_update(lio_localmap*, lio_ndt* target, const double pose_xyz[3], double update_distance, double radius, double key_frame_distance,
                        float leaf, int* n_keyframes, uint32_t* n_points);
int lio_localmap_download(lio_localmap*, float* out_xyzi, uint32_t cap);

/* ABI 19 -- the operator's pose hint on the device: GlobalLocalization::getEstimatePose (slam/localization/src/global_localization.cpp:196-262).
 * The key frames near the hint become the FAST_VGICP matcher's target without leaving HBM, the latest scan (already in HBM) is its source.
 *   nearest ........ mGraphKDTree->nearestKSearch over the key-frame positions with z = 0 on both sides (buildGraphKDTree), on the host: f32,
 *                    dx = pos_x - (float)x, dy = pos_y - (float)y, d2 = dx*dx + dy*dy; the min(k, frames) smallest (d2, id) in rising order --
 *                    equal distances go to the smaller id.  Returns the count; d2 may be NULL.
 *   gather ......... the named key frames' clouds back to back, in the order given, into a buffer of the local map by ONE launch, which also
 *                    sums z.  THE CHUNKED Z SUM (the project's rule; the reference adds sequentially, so the last bits differ -- the mean only
 *                    seeds a guess): the output is cut into chunks of 256 consecutive points; lane j of chunk c holds (double)z of point
 *                    256 c + j, or 0 past the end; a chunk's sum is the tree x[j] += x[j + s] for s = 128, 64, ..., 1; the chunk sums are
 *                    added in rising chunk order by one thread; the mean is that sum divided by n (on the host).  No floating-point atomics:
 *                    two runs give the same bits.  n_ids <= 16; ids may repeat; empty frames are allowed; a total of 0 is LIO_E_INVALID; a total
 *                    above the buffer (max(max_local_points + max_keyframe_points, 5 * max_keyframe_points)) is LIO_E_CAPACITY; a refused
 *                    call changes nothing (the previous gather is still there).
 *   z_mean ......... the same sum over any cloud in HBM (the hint's source), by the same rule.
 *   download_gather / gather_device  the last gather, to the host / where it lies (NULL before the first).
 *   store_frame / frame  two clouds kept with the local map as device copies (slot 0, 1; the module keeps the latest scan and the frame a hint
 *                    was matched with); n = 0 empties a slot.
 *   estimate_pose .. 1. the LIO_ESTIMATE_K = 5 nearest key frames to (hint[3], hint[7]), up to the first with d2 > 400;  2. gather -> target,
 *                    source from the device;  3. hint z = z_mean(target) - z_mean(source);  4. the guess is the hint rounded to f32;
 *                    5. lio_gicp_align with lio_estimate_matcher_params (the loop detector's coarse FAST_VGICP) -- `gicp` must be in voxel mode
 *                    with the loop parameters' voxel_resolution, DIRECT1;  6. not converged: result 0, out_T = the hint with the new z;
 *                    7. else lio_gicp_fitness_score(loop fitness_score_max_range): score < 5 -> out_T = the final transformation through f32,
 *                    score < 0.5 -> result 1;  8. no key frame within 20 m, only empty ones, or n_source = 0: result 0, out_T = the hint
 *                    untouched, LIO_OK.  A matcher error (a cloud below k points, over its max_points) is returned as it is, with result 0
 *                    and out_T = the hint.  400, 5.0 and 0.5 are the reference's.  There is no CPU path.
 * The report's stage times are HIP-event spans on the local map's stream; the matcher's stages run on the matcher's streams and are waited for
 * before the next event, so a span covers the stage's launches and the host work between them (the LM loop of align). */
#define LIO_ESTIMATE_K 5
typedef struct lio_estimate_report {
    int32_t n_ids, ids[LIO_ESTIMATE_K];
    uint32_t n_target, n_source;
    int32_t converged, iterations, result, pose_replaced; /* result: the reference's return value; pose_replaced: score < 5 */
    double z_mean_target, z_mean_source;
    double guess[16]; /* what the matcher started from (f32 values) */
    double score;     /* 0 when the matcher did not converge */
    double nearest_us /* host */, gather_us, set_target_us, set_source_us, z_source_us, align_us, fitness_us;
} lio_estimate_report;
int lio_localmap_nearest(lio_localmap*, const double xy[2], uint32_t k, int32_t* ids, float* d2);
int lio_localmap_gather(lio_localmap*, const int32_t* ids, uint32_t n_ids, uint32_t* n_points, double* z_mean);
int lio_localmap_z_mean(lio_localmap*, const void* d_xyzi, uint32_t n, double* z_mean);
int lio_localmap_download_gather(lio_localmap*, float* out_xyzi, uint32_t cap);
const void* lio_localmap_gather_device(lio_localmap*, uint32_t* n);
int lio_localmap_store_frame(lio_localmap*, int slot, const void* d_xyzi, uint32_t n);
const void* lio_localmap_frame(lio_localmap*, int slot, uint32_t* n);
void lio_estimate_matcher_params(lio_ndt_params* out);
int lio_localmap_estimate_pose(lio_localmap*, lio_gicp*, const void* d_source_xyzi, uint32_t n_source, const double hint[16], lio_estimate_report* report,
                               double out_T[16]);

/* ---------------------------------------------------------------------------------------------------------------
 * Dense-map export on the device: one cloud that grows over a drive (the reference's static g_accumulate_cloud,
 * slam/src/graph_utils.cpp:410, and g_map_config.points, :152-158), fed frame by frame and filtered as a whole.
 * The cloud lives in HBM; it grows geometrically when it has to, and a failed allocation returns an error and leaves it
 * unchanged.  NULL from lio_cloud_create without a device: there is no CPU fallback.
 * Appends (the per-frame bodies of accumulate_cloud, graph_utils.cpp:423-429, and export_points, :168-178): every point is
 *   - its intensity multiplied by intensity_scale unless that is 1 (numpy_to_pointcloud(points, 255.0), py_utils.cpp:102-116),
 *   - transformed by the row-major f64 matrix T as pcl::transformPointCloud(in, out, Matrix4d) does (f64, terms left to right, cast to f32;
 *     non-finite points too; T = NULL: identity),
 *   - kept only if z_min <= z <= z_max (compared in f64; NaN z is dropped) when z_band != 0 (export_points, graph_utils.cpp:173),
 *   - appended in input order.
 * ------------------------------------------------------------------------------------------------------------- */
typedef struct lio_cloud lio_cloud;
lio_cloud* lio_cloud_create(int device, uint64_t reserve_points);
void lio_cloud_destroy(lio_cloud*);
int lio_cloud_clear(lio_cloud*);                 /* save_accumulate_cloud's reset, graph_utils.cpp:444 */
int lio_cloud_size(lio_cloud*, uint64_t* n);
/* the scan's raw cloud as it stands (after lio_scan_upload and lio_scan_undistort_poses: undistortion_cloud, graph_utils.cpp:384-396); waits
 * for the append, so the scan may be reused at once */
int lio_cloud_append_scan(lio_cloud*, lio_scan*, const double T[16], float intensity_scale, int z_band, double z_min, double z_max);
int lio_cloud_append_host(lio_cloud*, const float* xyzi, uint64_t n, const double T[16], float intensity_scale, int z_band, double z_min, double z_max);
/* pcl::VoxelGrid::filter with setLeafSize(leaf, leaf, leaf) over the whole cloud, in place (save_accumulate_cloud, graph_utils.cpp:436-441):
 * the semantics of lio_scan_voxel_downsample (bbox of the finite points, the int32 overflow guard returning the input, one centroid per
 * occupied voxel as sequential f32 sums in ascending input index, ascending voxel index) for up to 2^31 - 1 points (PCL's int index range;
 * more: LIO_E_CAPACITY).  The sort scratch is allocated for the call and freed after it; *n_out (may be NULL) = points left. */
int lio_cloud_voxel_downsample(lio_cloud*, float leaf, uint64_t* n_out);
int64_t lio_cloud_download(lio_cloud*, float* xyzi, uint64_t cap);   /* the point count, or -(points) when cap is too small */
int lio_cloud_scratch_bytes(lio_cloud*, uint64_t* bytes);            /* peak device scratch lio_cloud_voxel_downsample takes at the current size */
/* device time (HIP events on the cloud's stream) of the last append (without the host-to-device copy of lio_cloud_append_host) and of the
 * last voxel grid (the kernel chain, without the scratch allocation) */
int lio_cloud_last_times(lio_cloud*, double* append_us, double* voxel_us);

/* -------------------------------------------------------------------------------------------------------------
 * Exact k nearest neighbours over a static cloud: the pcl::KdTreeFLANN<PointXYZRGB> of texture_mesh (slam/src/graph_utils.cpp:449-501,
 * FLANN's default L2_Simple<float>), as a device index (csrc/knn_index.hip).  NULL from lio_knn_index_create without a device: there is
 * no CPU fallback.
 *   - only points with three finite coordinates are indexed (PCL's isFinite filter in setInputCloud); indices refer to the input order;
 *   - distance = ((dx*dx) + dy*dy) + dz*dz in f32, d = p - q, every operation a separate IEEE operation;
 *   - the result is the k smallest distances in ascending (d2, index) order: ties at equal f32 distance go to the SMALLER input index
 *     (the project's rule: FLANN's own order among equal distances depends on its tree);
 *   - fewer than k indexed points: what there is (FLANN lowers k to the point count); a query with a non-finite coordinate: none;
 *   - up to 2^31 - 1 input points (PCL's int index; more: LIO_E_CAPACITY), any number of queries (the device takes them in chunks).
 * ------------------------------------------------------------------------------------------------------------- */
typedef struct lio_knn_index lio_knn_index;
lio_knn_index* lio_knn_index_create(int device);
void lio_knn_index_destroy(lio_knn_index*);
/* xyz: n x 3 f32 (host); rgb: n packed 0x??RRGGBB words or NULL; *n_finite (may be NULL) = points indexed.  Replaces any earlier build. */
int lio_knn_index_build(lio_knn_index*, const float* xyz, const uint32_t* rgb, uint64_t n, uint64_t* n_finite);
/* q: m x 3 f32 (host); 1 <= k <= 8; idx / d2: m x k, ascending (d2, idx); missing slots idx = -1, d2 = +inf */
int lio_knn_index_query(lio_knn_index*, const float* q, uint64_t m, int k, int32_t* idx, float* d2);
/* per query: floor(sum / count) of the r, g, b bytes of its (up to) k neighbours; count 0 -> 0, 0, 0.  rgb_out: m x 3 bytes.
 * LIO_E_STATE when the index holds points but was built without colours. */
int lio_knn_index_colour(lio_knn_index*, const float* q, uint64_t m, int k, uint8_t* rgb_out);
/* device time (HIP events on the index's stream, no host copies) of the last build and of the last query / colour call (all its chunks) */
int lio_knn_index_last_times(lio_knn_index*, double* build_us, double* query_us);

/* -------------------------------------------------------------------------------------------------------------
 * Ground extraction on the device (csrc/ground.hip): detect_ground of slam/src/graph_utils.cpp:329-382 with plane_clip (:285-297) and
 * normal_filtering (:299-327) -- the same stage as the mapping mode's floor detector, slam/backend/hdl_graph_slam/apps/
 * floor_detection_nodelet.cpp:79-193.  PCL is restated from its published algorithms (1.9.1); where its behaviour cannot be reproduced the
 * rule is this project's and is written here.  NULL from lio_ground_create without a device: there is no CPU fallback.
 *   clip     a point is kept iff x, y, z are finite and sensor_height - clip_low <= z < sensor_height + clip_high, z compared in f64
 *            (PlaneClipper3D with (0, 0, 1, .): inclusive, then negated, :337-338); input order kept.
 *   normals  (use_normal_filter != 0) the k = 10 nearest clipped points of every clipped point, itself first, by the rules of lio_knn_index
 *            (f32 distances, ties to the smaller index); centroid and 3 x 3 scatter about it in f64 over the neighbours in ascending
 *            (d2, index) order; the unit eigenvector n of the smallest eigenvalue by cyclic Jacobi in f64 (THE PROJECT'S RULE: PCL's eigen
 *            solver works in f32 and rounds differently); fewer than 3 neighbours: NaN, dropped.  Kept iff |n_z| > cos(normal_thresh_deg)|n|
 *            (:316-320); order kept.
 *   ransac   pcl::RandomSampleConsensus over SampleConsensusModelPlane, no refit.  THE PROJECT'S RULE for the draws (PCL's generator and
 *            shuffle are not reproducible): with mix(x) = { x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16 }
 *            on uint32 and s = mix(seed ^ 0x9E3779B9), draw j over N points uses r_t = mix(s + 3 j + t), t = 0, 1, 2 (mod 2^32):
 *              i0 = (r0 * N) >> 32;  i1 = (r1 * (N - 1)) >> 32, plus 1 if i1 >= i0;
 *              i2 = (r2 * (N - 2)) >> 32, plus 1 if i2 >= min(i0, i1), then plus 1 if i2 >= max(i0, i1)      (64-bit products)
 *            -- three distinct indices (lio_ground_draw computes them on the host).  The plane, every f32 operation rounded to nearest on
 *            its own (no fused multiply-add), in this order: a = p1 - p0, b = p2 - p0;
 *              c = (ay*bz - az*by, az*bx - ax*bz, ax*by - ay*bx);  l2 = (cx*cx + cy*cy) + cz*cz;  l = sqrt(l2);  n = c / l;
 *              d = -(((nx*p0x) + ny*p0y) + nz*p0z).
 *            A draw whose l2 is zero or not finite is bad and counts as PCL counts a skipped sample.  The score of a plane is the number
 *            of points with |((nx*x + ny*y) + nz*z) + d| < (float)distance_threshold in f32.  The loop is ransac.hpp's, in draw order:
 *            while (iterations < k && skipped < 10 max_iterations): a bad draw -> ++skipped; else a strictly larger count becomes the best
 *            and k = log(1 - probability) / log(clamp(1 - pow(best / N, 3), eps, 1 - eps)), then ++iterations and stop once
 *            iterations > max_iterations.  The device scores 64 draws per launch; draws past the loop's end are discarded.
 *   result   none when fewer than min_points points are left after the filter, when the best plane has fewer than min_points inliers, or
 *            when |n_z| < cos(floor_normal_thresh_deg) (:342, :356, :366-370); else the coefficients, negated if n_z < 0 (:373-375), and
 *            the inliers of the `<` test in order (the points as they came in, intensity included).
 * ------------------------------------------------------------------------------------------------------------- */
typedef struct lio_ground lio_ground;
typedef struct lio_ground_params {
    double sensor_height;            /* 0 */
    double clip_low;                 /* height_clip_range_low */
    double clip_high;                /* height_clip_range_high */
    int32_t use_normal_filter;       /* the floor detector's use_normal_filtering; detect_ground always filters */
    double normal_thresh_deg;        /* 20 */
    int32_t k;                       /* neighbours of the normal estimation; only 10 is built */
    double distance_threshold;       /* 0.1, compared as f32 */
    int32_t min_points;              /* floor_pts_thresh = 1024 */
    double floor_normal_thresh_deg;  /* 10 */
    int32_t max_iterations;          /* 1000 (PCL's default) */
    double probability;              /* 0.99 (PCL's default) */
    uint32_t seed;                   /* of the draws */
} lio_ground_params;
/* preset 0: detect_ground (graph_utils.cpp:330-333: clip 1.5 / 1.5); preset 1: the floor detector's initialize_params
 * (floor_detection_nodelet.cpp:38-46: clip 2.0 / 1.0) */
void lio_ground_default_params(lio_ground_params*, int preset);
/* draw j of a run with `seed` over n >= 3 points, by the rule above (host only; n < 3: zeros) */
void lio_ground_draw(uint32_t seed, uint32_t j, uint32_t n, uint32_t out[3]);
lio_ground* lio_ground_create(int device);
void lio_ground_destroy(lio_ground*);
/* detect_ground on the scan's raw cloud as it stands (after lio_scan_upload / lio_scan_undistort_poses).  *found = 1 and coeffs = (nx, ny, nz,
 * d) with n_z >= 0 when there is a floor.  replace != 0 and a floor: the scan's raw cloud becomes the inlier cloud (extract.filter(*cloud),
 * :377-380), which lio_cloud_append_scan then appends; otherwise the scan is left as it is.  The counts may be NULL. */
int lio_ground_detect_scan(lio_ground*, lio_scan*, const lio_ground_params*, int replace, int* found, float coeffs[4], uint32_t* n_clipped,
                           uint32_t* n_filtered, uint32_t* n_inliers);
/* the same for n host points (x, y, z, intensity) */
int lio_ground_detect_host(lio_ground*, const float* xyzi, uint64_t n, const lio_ground_params*, int* found, float coeffs[4], uint32_t* n_clipped,
                           uint32_t* n_filtered, uint32_t* n_inliers);
/* the stages of the last call; each returns the number of items, or -(items) when cap is too small.
 * indices: positions in the input cloud of the clipped (stage 0), the filtered (1) and the inlier points (2), ascending;
 * normals: n x 3, one per clipped point (nothing when the filter was off); inliers: the inlier cloud, n x 4;
 * draws: every draw the device scored (whole batches of 64; lio_ground_last_run tells how many the loop used): its three indices into the
 * filtered points, its count (0xFFFFFFFF: a bad draw) and its plane (NaN for a bad draw); any of the three arrays may be NULL */
int64_t lio_ground_download_indices(lio_ground*, int stage, uint32_t* out, uint64_t cap);
int64_t lio_ground_download_normals(lio_ground*, float* out_n3, uint64_t cap);
int64_t lio_ground_download_inliers(lio_ground*, float* xyzi, uint64_t cap);
int64_t lio_ground_download_draws(lio_ground*, uint32_t* triples, uint32_t* counts, float* planes, uint64_t cap);
/* the replay of the last call: iterations and skipped draws of ransac.hpp's loop, draws consumed, and the winning draw (-1: none) */
int lio_ground_last_run(lio_ground*, int* iterations, int* skipped, int* draws_used, int* winner);
/* device time (HIP events on the detector's stream) of the last call: clip + k-NN + normals + filter, and RANSAC with the inlier selection
 * (the host's replay between the batches included) */
int lio_ground_last_times(lio_ground*, double* filter_us, double* ransac_us);

/* -------------------------------------------------------------------------------------------------------------
 * Bird's-eye intensity image of a dense map on the device (csrc/bev.hip): tools/postprocessing/convert_cloud_image.py, function by function,
 * under numpy 2 promotion rules (Python scalars are weak, f32 arrays stay f32).  Where the reference is undefined or cannot be followed the
 * rule is THE PROJECT'S and is marked so.  NULL from lio_bev_create without a device: there is no CPU fallback.
 *   bounds   (load_pointcloud) PROJECT: points whose x, y or intensity is not finite are dropped first and counted (the reference's min / max
 *            turn NaN); none left: LIO_E_INVALID.  x_min .. y_max are the f32 extremes; image_w = ceil((x_max - x_min) ppm) + 1 in f64, image_h
 *            likewise; xs = rint((x - x_min) * (float)ppm), ys = rint((-(y - y_max)) * (float)ppm) in f32, ties to even.  The pixel key is
 *            ys image_w + xs in 32 bits.  PROJECT: a side above 2^22 pixels or image_w image_h above 2^32 - 1 is LIO_E_CAPACITY (the key never
 *            wraps), and so is a coordinate that leaves the image.
 *   noise    (filter_noise) the m finite points in ascending (intensity, input index) order, -0.0 equal to +0.0 (PROJECT: numpy's argsort
 *            leaves the order of equal intensities open); ranks [int(m 0.01), int(m 0.999)) (f64 products) are kept, in that order.
 *   means    (scatter) occupied pixels in ascending key order; intensity and z of a pixel are f32 sums over its kept points taken one after
 *            the other in that (intensity, input index) order, divided by the f32 count.
 *   nodes    (convert) P = int(window ppm), h = int(P / 2), q = int(h / 2); the image is padded to W = int((image_w + h) / h) h, H likewise;
 *            nodes at xi = 0, h, .., W and yi = 0, h, .., H; node number (xi / h) (H / h + 1) + yi / h.  A node runs when more than 100
 *            occupied pixels lie in [xi - P, xi + P] x [yi - P, yi + P] (PROJECT: and one of them has a value in [0, 65535]; the reference
 *            divides by zero there).  P < 2 is LIO_E_INVALID (the reference's range() has step 0).
 *   equalise (intensity_normalize) v = I * 65535 in f32.  numpy's histogram with 1024 bins over [0, 65535]: edges e_i = f32(i * 65535 / 1024),
 *            bin = the f32 estimate (v / 65535) * 1024 truncated, stepped down or up once against the edges, values outside ignored, the last
 *            bin closed; density n_i / f64(e_(i+1) - e_i in f32) / N, its cumulative sum in f64 one bin after the other, cdf = (65535 cdf)
 *            / cdf[1023].  interp(v): cdf[0] below 0, cdf[1023] from e_1023 on, cdf[j] at an edge, else slope_j (v - e_j) + cdf[j] in f64
 *            with slope_j = (cdf[j+1] - cdf[j]) / (e_(j+1) - e_j); amplify = interp(v) / f64(max(v, 0.001f)); value(c) = f64(v) *
 *            min(amplify, c).
 *            PROJECT (numpy's pairwise f32 / f64 sums cannot be followed in parallel): a mean is sum(t) / count with every term
 *            t = rint(clamp(x, -2^23, 2^23) * 2^16) as a 64-bit integer (NaN: 0) -- exact, so the same in any order.  mean(v) is that sum
 *            over f64(v), rounded as f32((S / 2^16) / count); c_0 = f32(20480 / mean) and c_(k+1) = c_k + 0.1f in f32 when c_0 > 1, else
 *            c_0 = 1.0 and c_(k+1) = c_k + 0.1 in f64 (Python's float, as max(1.0, .) returns it); the table ends at the first
 *            c_k >= 120.  The step is the first k at which the table ends or sum(t(value(c_k))) >= 20480 * 2^16 * count: by bisection
 *            when no v is negative (the sum is then monotone in c), by the reference's linear scan otherwise.  The node's result for a
 *            pixel is f32(clip(value(c_step), 0, 65535)) (NaN: 0).
 *   render   (convert, bev_generate) a pixel takes the result of the last running node, xi major and yi minor, whose inner region
 *            [xi - q, xi + q] x [yi - q, yi + q] holds it; a pixel no running node holds keeps its raw mean I (not scaled: it renders as grey
 *            0 or 1).  g = rint(value) in f32, ties to even (PROJECT: clamped to [0, 65535]; the reference indexes out of range), and the
 *            image is grey[g] at (ys, xs) of the zero-filled H x W uint16 image, grey[i] = trunc(t_i * 65535) in f64 with
 *            t_i = i * (1 / 65535), t_65535 = 1 (matplotlib's 'gray' resampled to 65536 entries; 88 entries are i - 1).
 * ------------------------------------------------------------------------------------------------------------- */
typedef struct lio_bev lio_bev;
typedef struct lio_bev_info {
    uint32_t n_in, n_dropped;        /* points given; points dropped as not finite */
    uint32_t n_kept, rank_lo, rank_hi; /* the noise filter's kept ranks [rank_lo, rank_hi) of the finite points */
    uint32_t n_pixels;               /* occupied pixels */
    uint32_t image_w, image_h;       /* load_pointcloud's size */
    uint32_t padded_w, padded_h;     /* the image's size (after lio_bev_convert) */
    int32_t patch, half_patch, quarter_patch;
    uint32_t nodes_x, nodes_y;
    uint32_t reserved;
    double pixel_per_meter, x_min, x_max, y_min, y_max;
} lio_bev_info;
lio_bev* lio_bev_create(int device);
void lio_bev_destroy(lio_bev*);
/* load_pointcloud + filter_noise + scatter over n host points (x, y, z, intensity), or over the points of a lio_cloud where they lie */
int lio_bev_preprocess_host(lio_bev*, const float* xyzi, uint64_t n, double pixel_per_meter);
int lio_bev_preprocess_cloud(lio_bev*, lio_cloud*, double pixel_per_meter);
/* a pixel list from elsewhere instead (convert's arguments): n strictly ascending keys ys image_w + xs with their intensities (z may be NULL) */
int lio_bev_upload_pixels(lio_bev*, const uint32_t* keys, const float* intensity, const float* z, uint64_t n, uint32_t image_w, uint32_t image_h);
/* convert + bev_generate over the handle's pixel list */
int lio_bev_convert(lio_bev*, double window, double pixel_per_meter);
int lio_bev_get_info(lio_bev*, lio_bev_info* out);
/* the stages of the last calls; each returns the number of items, or -(items) when cap (in items) is too small.
 * pixel_coords: (xs, ys) per input point, (-1, -1) for a dropped one; kept: input indices of the kept points in (intensity, index) order;
 * pixels: key, mean intensity and mean z per occupied pixel (any array may be NULL); nodes: occupied pixels in the window, step (-1: the node
 * did not run) and clip limit per node (any may be NULL); equalised: the f32 value per occupied pixel before rint; image: padded_h x padded_w */
int64_t lio_bev_download_pixel_coords(lio_bev*, int32_t* xy, uint64_t cap);
int64_t lio_bev_download_kept(lio_bev*, uint32_t* idx, uint64_t cap);
int64_t lio_bev_download_pixels(lio_bev*, uint32_t* keys, float* intensity, float* z, uint64_t cap);
int64_t lio_bev_download_nodes(lio_bev*, uint32_t* count, int32_t* step, double* clip, uint64_t cap);
int64_t lio_bev_download_equalised(lio_bev*, float* out, uint64_t cap);
int64_t lio_bev_download_image(lio_bev*, uint16_t* out, uint64_t cap);
/* the grey table above (host only) */
void lio_bev_grey_table(uint16_t out[65536]);
/* device time (HIP events on the handle's stream) of the last preprocess (the two host read-backs included) and of the last convert */
int lio_bev_last_times(lio_bev*, double* preprocess_us, double* convert_us);

/* -------------------------------------------------------------------------------------------------------------
 * The mapping mode's key frames on the device (csrc/keyframe.hip): HdlGraphSlamNodelet::cloud_callback
 * (slam/backend/hdl_graph_slam/apps/hdl_graph_slam_nodelet.cpp:163-246, "NL" below; constants NL:44-45, 61-65) and the two filters
 * SLAM::runMappingThread puts an elected frame through (slam/src/slam.cpp:105-108, 400-411).  The pose graph, loop closure and the GNSS / floor
 * edges are not built: odom -> map is the identity.  NULL from lio_keyframer_create without a device: there is no CPU fallback.
 *   decide   KeyframeUpdater::is_update (include/hdl_graph_slam/keyframe_updater.hpp:60-75): delta = prev^-1 * pose, dx = |t|,
 *            da = AngleAxis(R).angle * 180 / pi in f64, both then STORED AS f32 (is_update's float& arguments) and compared as doubles:
 *            need = !(dx < D / 2 && da < A / 2), must = need && (dx >= 1.5 D || da >= 1.5 A).  update() (:42-58) adds the f64 dx to the
 *            accumulated distance and moves prev.  The angle is taken through the quaternion, 2 atan2(|vec|, |w|), as Eigen does.
 *   frame    an empty cloud leads to nothing (NL:165).  First frame (NL:169-176): update, VoxelGrid(resolution) of the cloud as it came (not
 *            undistorted), transformed by the odometry -- pcl::transformPointCloud with a Matrix4d: f64, terms left to right, cast to f32, the
 *            rule of lio_cloud_append_* -- which becomes the local map; no key frame.  Later frames: nothing unless need; undistortion
 *            (lio_scan_undistort_delta with delta.cast<float>() and scan_period when no poses are given, lio_scan_undistort_poses otherwise,
 *            NL:186-191), VoxelGrid(resolution), then the score.
 *   score    calc_fitness_score(local_map, cloud, odom, nr, 1.0) (src/hdl_graph_slam/information_matrix_calculator.cpp:110-138): the cloud
 *            transformed by odom.cast<float>() in f32 (the rule of lio_ndt_overlap_score), the exact nearest local-map point by the rules of
 *            lio_knn_index (d2 = ((dx*dx) + dy*dy) + dz*dz in f32), squared distances <= fitness_range summed in f64, divided by their number
 *            nr; DBL_MAX when nr = 0.  The sum is taken per 256 consecutive points in a fixed order and then over those records in order:
 *            run-to-run identical.  inlier = float(nr) / n.  The candidate replaces the best one iff
 *            0.8 score + 0.2 (1 - inlier) <= 0.8 best_score + 0.2 (1 - best_inlier); best_score starts at DBL_MAX, best_inlier at 0, and
 *            best_inlier is NOT reset with best_score (NL:224).
 *   must     update; the best frame is emitted -- its downsampled cloud through the filters below, its odometry pose, its header stamp, the
 *            accumulated distance -- average_score is updated, best_score reset; every max(1, round(local_map_distance / D))-th key frame
 *            the best cloud (before the filters), transformed by its pose (Matrix4d rule), is appended to the local map, points are dropped
 *            from the FRONT down to local_map_cap, and the tree is rebuilt (NL:211-235).
 *   filters  pcl::RadiusOutlierRemoval(radius, min_neighbours) restated from PCL 1.9.1's published radius_outlier_removal.hpp: the search
 *            includes the query point, and a point stays iff MORE THAN min_neighbours points, itself included, lie within the radius.
 *            THE PROJECT'S RULES: the distance is lio_knn_index's f32 d2; "within" is d2 <= (float)(radius * radius); coincident points
 *            count; rows with a non-finite coordinate are dropped and counted.  Then pointsDistanceFilter(0, key_frame_range)
 *            (slam/common/slam_utils.cpp:236-241): kept iff 0 < |x| < range && 0 < |y| < range, the f32 absolute values compared strictly
 *            with the doubles (a point with x == 0 goes).  The survivors keep the input's order.
 * ------------------------------------------------------------------------------------------------------------- */
typedef struct lio_keyframer lio_keyframer;
typedef struct lio_keyframer_params {
    double key_frame_distance;   /* D: init_slam's dist_threshold (1.0) */
    double key_frame_degree;     /* A: init_slam's degree_threshold (10.0) */
    double resolution;           /* VoxelGrid leaf, used as f32 (0.2) */
    double key_frame_range;      /* init_slam's frame_range (50.0); <= 0: no range filter */
    double scan_period;          /* 0.1, slam.cpp:103 */
    double radius;               /* 1.0, slam.cpp:106 */
    int32_t min_neighbours;      /* 3, slam.cpp:107 */
    uint32_t local_map_cap;      /* ODOMETRY_LOCAL_MAP_NUM = 100000 */
    double local_map_distance;   /* ODOMETRY_LOCAL_MAP_DIST = 2.0 */
    double fitness_range;        /* 1.0 (a squared distance), NL:202 */
} lio_keyframer_params;
typedef struct lio_keyframe_report {
    int32_t first, need, must;   /* the first frame; is_update's two flags */
    int32_t elected, emitted;    /* the frame became the best candidate; a key frame went to the queue */
    uint32_t nr, n_downsampled;  /* calc_fitness_score's nr; points after the VoxelGrid */
    uint32_t local_map_size;     /* points of the local map after the call */
    double dx, da;               /* is_update's f32 values */
    double score;                /* DBL_MAX: none */
    double accum_distance, average_score;
} lio_keyframe_report;
/* keyframe_updater.hpp:60-75, host only (no device needed); prev and pose are row-major 4 x 4 rigid transforms; any output may be NULL */
int lio_keyframe_decide(const double prev[16], const double pose[16], double dist_threshold, double degree_threshold, int* need, int* must, double* dx,
                        double* da);
void lio_keyframer_default_params(lio_keyframer_params*);
/* onInit (NL:56-110); params NULL = the defaults */
lio_keyframer* lio_keyframer_create(int device, const lio_keyframer_params* params);
void lio_keyframer_destroy(lio_keyframer*);
/* back to onInit's state: the next frame is a first frame, the local map and the queue are empty; device memory is kept */
int lio_keyframer_reset(lio_keyframer*);
/* cloud_callback (NL:163-246) for one frame: n points (x, y, z, intensity) with their stamps (us since the header stamp), the frame's header
 * stamp, its odometry pose, and either the frame's delta pose start^-1 * end (n_poses == 0: frame.points->T, NL:186-188) or the frame's pose
 * list as lio_scan_undistort_poses takes it (absolute stamps, n_poses x 16 doubles; NL:190).  Synchronous.  *report may be NULL. */
int lio_keyframer_push_host(lio_keyframer*, const float* xyzi, const uint32_t* stamp_us, uint32_t n, uint64_t header_stamp_us, const double odom[16],
                            const double delta[16], const uint64_t* pose_stamp_us, const double* poses, uint32_t n_poses, lio_keyframe_report* report);
/* the reference's keyframe_queue (NL:215-219, unbounded) after the two filters of slam.cpp:400-411: a FIFO */
int lio_keyframer_pending(lio_keyframer*);
/* the oldest key frame: its points (the count, or -(count) when xyzi is NULL or cap is too small -- the frame then stays queued; LIO_E_STATE when
 * none is pending),
 * its odometry pose, header stamp and accumulated distance, and the sizes of its cloud before the filters and after the radius filter */
int64_t lio_keyframer_pop(lio_keyframer*, float* xyzi, uint64_t cap, double pose[16], uint64_t* stamp_us, double* accum_distance, uint32_t* n_before_filters,
                          uint32_t* n_after_radius);
/* stage doors.  The radius outlier filter over n host points on the handle's device: the kept input indices, ascending (the count, or -(count)
 * when cap is too small); lio_keyframe_filter_host: the same followed by the range filter (range <= 0: none), as an elected frame goes through
 * both.  lio_keyframer_fitness_host: calc_fitness_score of a host cloud against the handle's local map.  lio_keyframer_append_local_map_host:
 * the local map's append (transform by T, drop from the front, rebuild the tree) for a host cloud; returns the local map's size.
 * lio_keyframer_download_local_map: the count, or -(count). */
int64_t lio_radius_outlier_host(lio_keyframer*, const float* xyzi, uint64_t n, double radius, int min_neighbours, uint32_t* keep_idx, uint64_t cap,
                                uint32_t* n_dropped_nonfinite);
int64_t lio_keyframe_filter_host(lio_keyframer*, const float* xyzi, uint64_t n, double radius, int min_neighbours, double range, uint32_t* keep_idx, uint64_t cap,
                                 uint32_t* n_after_radius, uint32_t* n_dropped_nonfinite);
int lio_keyframer_fitness_host(lio_keyframer*, const float* xyzi, uint32_t n, const double T[16], double* score, uint32_t* nr);
int lio_keyframer_append_local_map_host(lio_keyframer*, const float* xyzi, uint32_t n, const double T[16]);
int64_t lio_keyframer_download_local_map(lio_keyframer*, float* xyzi, uint64_t cap);
/* device time (HIP events on the handle's stream) of the stages of the last call: upload + undistortion + VoxelGrid, the fitness score, the two
 * filters with the download, the local map's append and rebuild; 0 for a stage that did not run */
int lio_keyframer_last_times(lio_keyframer*, double* candidate_us, double* fitness_us, double* filters_us, double* ring_us);

/* -------------------------------------------------------------------------------------------------------------
 * Loop detection over the key frames on the device (csrc/loop.hip): hdl_graph_slam::LoopDetector
 * (slam/backend/hdl_graph_slam/include/hdl_graph_slam/loop_detector.hpp, "LD" below).  The pose graph is not built: the detector stops at the
 * loop edge -- the pair, the relative pose, the score and the information matrix -- which is what the reference hands to add_se3_edge.
 * NULL from lio_loop_create without a device: there is no CPU fallback.
 *   candidates  find_candidates (LD:106-140), statement for statement: nothing when new.accum - last_edge_accum < distance_from_last_edge_thresh;
 *               a frame is passed over when new.accum - k.accum < accum_distance_thresh (strict), when k.accum - (accum of the last ACCEPTED
 *               candidate, -100 at the start) < distance_keyframe_thresh, or when the planar distance of the two estimates is > distance_thresh
 *               (strict: a frame exactly at the threshold stays).
 *   detect      detect (LD:69-93) over the queued new frames in order: a frame is passed over when its accum - (accum of the last new frame that
 *               was matched, 0 at the start of every call) < distance_new_keyframe_thresh; then matching; afterwards the new frames join the
 *               key frames (optimization_timer_callback, apps/hdl_graph_slam_nodelet.cpp:623).
 *   matching    (LD:148-219) the TARGET is the new frame, the sources are the candidates.  guess = new^-1 * candidate in f64, both rotations
 *               renormalised through a quaternion first, cast to f32, then guess(2,3) = 0.  Coarse: FAST_VGICP (src/hdl_graph_slam/registrations.cpp:56-66:
 *               resolution 1.0, translation epsilon 0.1, rotation epsilon 0.1, 64 iterations, k = 20, DIRECT1) for ALL candidates in one batch
 *               with LsqRegistration's LM loop (lsq.h) on the device.  A candidate that did not converge is skipped; a candidate replaces the
 *               best unless score > best_score (an equal score takes the LATER one); best_score > 2 fitness_score_thresh ends the frame.  Fine:
 *               FAST_GICP (registrations.cpp:33-42; max correspondence distance fine_max_corr_dist = 0.5, LD:59) from the coarse result of the
 *               best; not converged, or score > fitness_score_thresh, ends the frame; otherwise last_edge_accum_distance = new.accum.
 *   fitness     pcl::Registration::getFitnessScore(max_range), restated from PCL 1.9.1's published registration.hpp (PCL is not in the tree): the
 *               source transformed by the f32 final transformation (pcl::transformPointCloud with a Matrix4f: terms left to right), the exact
 *               nearest target point, d2 <= max_range applied to the SQUARED distance (fitness_score_max_range = 25 is 5 m), the sum divided by
 *               the number nr of such points, DBL_MAX when nr = 0.  THE PROJECT'S RULES: lio_knn_index's f32 d2 = ((dx*dx) + dy*dy) + dz*dz, ties to
 *               the smaller index; f64 sums taken per 256 consecutive points in a fixed order and then over those records in order (the
 *               keyframer's rule): run-to-run identical.
 *   information InformationMatrixCalculator::calc_information_matrix(const double&) with weight() and the constructor's constants
 *               (include/hdl_graph_slam/information_matrix_calculator.hpp:44-47, src/hdl_graph_slam/information_matrix_calculator.cpp:10-21,50-63):
 *               var_gain_a 20, stddev x in [0.1, 5], q in [0.05, 0.2], its own fitness_score_thresh 0.5; w_x and w_q are rounded to f32 (the
 *               reference's float locals) before the identity's diagonal is divided by them.
 *   bank        a key frame is uploaded once; its regularised k-NN covariances (calculate_covariances, fast_gicp_impl.hpp:244-303, the path of
 *               lio_gicp_set_source) are computed once and stay resident with the cloud (both in the caller's point order) for the frame's
 *               life -- the reference's setInputSource computes them again every time a frame is a candidate.  A hash grid's own point order is
 *               the arrival order inside a cell and differs from one insertion to the next; every sum over a frame (cost, fitness, the fold of
 *               a target's Gaussian voxels) therefore runs in the frame's own order, so the same frames give the same bits after a reset.
 * THE PROJECT'S RULES of the batch: every slot folds its own workgroup partials in workgroup order with f64 accumulators (the fold of the
 * single-pair lio_gicp_align); no floating-point atomics; a slot's numbers do not depend on its neighbours or on its place in the batch.
 * DEVIATIONS: the coarse matcher is the reference's non-CUDA branch (FAST_VGICP; the CUDA build's NDT_CUDA coarse step is not offered), and
 * setMaxProcessTime(50000) does not apply (a wall-clock rule, as for lio_ndt_align_batch).  A THIRD, found while the vectors were recorded: when
 * NO source point of a candidate meets a voxel, H and b are zero; Eigen's LDLT answers a null step, which the reference accepts, and it reports
 * the untouched guess as CONVERGED and scores it.  lsq.h's ldlt_solve6 (shared with lio_ndt_align / lio_gicp_align) reports the zero pivot and
 * the alignment ends NOT converged, here as in the single-pair path: the detector skips such a candidate.
 * ------------------------------------------------------------------------------------------------------------- */
typedef struct lio_loop lio_loop;
typedef struct lio_loop_params {
    double distance_thresh;                 /* 15 (LD:43) */
    double accum_distance_thresh;           /* 25 */
    double distance_from_last_edge_thresh;  /* 15 */
    double distance_new_keyframe_thresh;    /* 2 */
    double distance_keyframe_thresh;        /* 2 */
    double fitness_score_max_range;         /* 25, compared with a squared distance (LD:49) */
    double fitness_score_thresh;            /* 1.5 */
    double fine_max_corr_dist;              /* 0.5 (LD:59) */
    double voxel_resolution;                /* 1.0 (registrations.cpp:59) */
    double coarse_translation_epsilon;      /* 0.1 */
    double coarse_rotation_epsilon_deg;     /* 0.1 */
    double fine_translation_epsilon;        /* 0.01 (registrations.cpp:37) */
    double fine_rotation_epsilon_deg;       /* 1e-2 (LsqRegistration's default, lsq_registration_impl.hpp:24) */
    int32_t max_iterations;                 /* 64 */
    int32_t k_correspondences;              /* 20 */
    float grid_resolution;                  /* cell of the hash grids the exact searches walk (1.0); a speed knob, never a result */
    uint32_t max_points;                    /* largest key frame taken (65536) */
    uint32_t max_candidates;                /* candidates aligned per launch set (64); more go through in further sets, same results */
    uint32_t pad;
} lio_loop_params;
typedef struct lio_loop_edge {
    int32_t key1, key2;          /* the new frame; the matched earlier frame */
    float relative_pose[16];     /* getFinalTransformation of the fine matcher, row-major: key2's frame -> key1's frame */
    double score;                /* the fine fitness */
    double information[36];      /* lio_loop_information_matrix(score) */
} lio_loop_edge;
#define LIO_LOOP_FOUND 0
#define LIO_LOOP_NO_CANDIDATE 1          /* the last-edge gate, or no earlier frame passed find_candidates */
#define LIO_LOOP_COARSE_SCORE 2          /* no candidate converged, or the best coarse score > 2 fitness_score_thresh */
#define LIO_LOOP_FINE_NOT_CONVERGED 3
#define LIO_LOOP_FINE_SCORE 4            /* fine score > fitness_score_thresh */
typedef struct lio_loop_report {
    int32_t new_id;              /* the last new frame that reached matching; -1: none since the handle was made / reset */
    int32_t n_candidates;
    int32_t best;                /* index into the candidate list; -1: none */
    int32_t fine_converged, fine_iterations;
    int32_t reason;              /* LIO_LOOP_* */
    int32_t coarse_rounds;       /* launch sets of the coarse batch (evaluations + LM step); 0: nothing was launched */
    int32_t pad;
    double best_score;           /* coarse; DBL_MAX: none */
    double fine_score;           /* DBL_MAX: not run or nr = 0 */
} lio_loop_report;
void lio_loop_default_params(lio_loop_params*);
/* host only (no device needed).  find_candidates over n key frames (accumulated distance, planar position of the estimate) for a new frame:
 * the indices of the candidates, ascending; the count, or -(count) when cap is too small */
int lio_loop_find_candidates(const double* accum, const double* pos_xy, uint32_t n, double new_accum, const double new_xy[2], double last_edge_accum,
                             const lio_loop_params* params, int32_t* out_idx, uint32_t cap);
int lio_loop_information_matrix(double fitness_score, double out36[36]);
/* params NULL = the defaults */
lio_loop* lio_loop_create(int device, const lio_loop_params* params);
void lio_loop_destroy(lio_loop*);
/* no key frames, no edges, last_edge_accum_distance = 0; scratch memory is kept */
int lio_loop_reset(lio_loop*);
/* a key frame into the bank and the new_keyframes queue: the id (0, 1, ...), LIO_E_INVALID for n < k (as lio_gicp_set_*), LIO_E_CAPACITY for
 * n > max_points.  pose = node->estimate(), row-major 4 x 4 */
int lio_loop_add_keyframe_host(lio_loop*, const float* xyzi, uint32_t n, const double pose[16], double accum_distance);
int lio_loop_set_pose(lio_loop*, int id, const double pose[16]);
/* a frame leaves the matching for good (graph_del_vertex, hdl_graph_slam_nodelet.cpp:868-891, erases the key frame from `keyframes`, the list
 * LoopDetector::detect searches): lio_loop_detect passes it over as a new frame and leaves it out of find_candidates as if it had never been
 * added, the stage doors (lio_loop_align_candidates, lio_loop_align_fine, lio_loop_pair_information, lio_overlap_gate_batch, _align_pairs,
 * _accumulate) answer LIO_E_INVALID for it as for an unknown id, and lio_overlap_detect drops it from the reference list -- so it is neither a
 * candidate nor a neighbour in the accumulated cloud -- and gives it no candidate as a new frame.  The slot, the id and the device storage stay:
 * no other frame's id moves, lio_loop_set_pose and lio_loop_download_keyframe still take the id, edges found earlier stay in lio_loop_edges.
 * LIO_E_INVALID for an unknown or already retired frame */
int lio_loop_retire(lio_loop*, int frame);
int lio_loop_num_keyframes(lio_loop*, int* n_queued);
/* a frame's resident cloud (the order it was added in) and covariances (xx, xy, xz, yy, yz, zz); the count, or -(count) when cap is too small */
int lio_loop_download_keyframe(lio_loop*, int id, float* xyzi, double* cov6, uint32_t cap);
/* detect over the queued frames; the loops of THIS call into out_loops.  The count, or -(count) when cap is too small: the call has then done its
 * work all the same and the edges are read with lio_loop_edges, which returns every edge since the last reset by the same convention.  On a
 * device error (a negative LIO_E_* code) the queue is emptied as well: the frame that failed and those behind it become key frames that were
 * never matched, the edges found before it stay, and a repeated call does not match the same frames twice */
int lio_loop_detect(lio_loop*, lio_loop_edge* out_loops, uint32_t cap);
int lio_loop_edges(lio_loop*, lio_loop_edge* out, uint32_t cap);
/* of the last new frame that reached matching; per candidate (arrays of cap entries, any may be NULL): id, converged, iterations, coarse score
 * (DBL_MAX where it was not taken).  The number of candidates, or -(number) when cap is too small (the record is still filled) */
int lio_loop_last_report(lio_loop*, lio_loop_report* report, int32_t* candidate_ids, int32_t* converged, int32_t* iterations, double* scores, uint32_t cap);
/* device time (HIP events) summed over the last detect call: target build (grid, voxels, index), coarse batch, fitness, fine step; and of the
 * last bank insert */
int lio_loop_last_times(lio_loop*, double* insert_us, double* target_us, double* coarse_us, double* fitness_us, double* fine_us);
/* stage door: the coarse batch and the fitness on their own.  n alignments of bank frames source_ids[] against bank frame target_id from
 * guesses (n x 16 f64, used as given); per job the final f64 transform, iterations, converged, fitness score (DBL_MAX when nr = 0 or not
 * converged) and nr.  Any output may be NULL */
int lio_loop_align_candidates(lio_loop*, int target_id, const int32_t* source_ids, uint32_t n, const double* guesses, double* out_T, int32_t* iterations,
                              int32_t* converged, double* scores, uint32_t* nr);
/* stage door: the fine matcher (FAST_GICP at fine_max_corr_dist) and its fitness for one pair of bank frames */
int lio_loop_align_fine(lio_loop*, int target_id, int source_id, const double guess[16], double out_T[16], int32_t* iterations, int32_t* converged, double* score,
                        uint32_t* nr);

/* the fitness score and information matrix of two bank frames under a given relative pose: InformationMatrixCalculator::calc_information_matrix(
 * cloud1, cloud2, relpose) (information_matrix_calculator.cpp:25-47, 71-102).  Frame id2 is transformed by relpose.cast<float>() against frame id1's
 * exact nearest neighbours; max_range = DBL_MAX, so every point with a neighbour counts; sums and ties by the fitness rules above; the score
 * then goes through lio_loop_information_matrix.  score, nr, info36 may be NULL */
int lio_loop_pair_information(lio_loop*, int id1, int id2, const double relpose[16], double* score, uint32_t* nr, double info36[36]);

/* -------------------------------------------------------------------------------------------------------------
 * Overlap detection between two maps on the device (csrc/overlap.hip): OverlapDetector of the reference's map merge
 * (slam/localization/include/overlap_merge.hpp, "OM" below; its caller is MapLoader::mergeMapSLAM, slam/localization/src/map_loader.cpp:82-169).
 * The handle works over a lio_loop bank: the key frames of BOTH maps are added with lio_loop_add_keyframe_host and addressed by bank id; poses
 * are the bank's (lio_loop_set_pose); the coarse matcher's parameters are the bank's.  The bank outlives the handle's use and is not owned by it.
 *   candidates  find_candidates (OM:113-145): the knn nearest key-frame positions by rising distance; the same id and an id already connected
 *               to the new one are passed over; d2 < distance_thresh^2 (strict); connection_count >= candidate_link_dist; at most
 *               max_candidate_num.  THE PROJECT'S RULES (FLANN leaves them open): positions rounded to f32 (pcl::PointXYZ),
 *               d2 = ((dx*dx) + dy*dy) + dz*dz in f32, equal distances go to the smaller index.
 *   connection_count  get_connection_count (OM:265-296), statement for statement: LEVELS of a breadth-first walk are counted, not hops; a node
 *               is marked visited when it is popped, so it can be queued more than once; the walk ends at count >= max_count (max_count > 0)
 *               and returns the count reached when the queue runs dry -- a new map whose component is shallower than candidate_link_dist
 *               levels from the new frame therefore yields no candidate.  That is the reference's behaviour and is kept.
 *   gate        calc_fitness_score (OM:225-263): the target filtered by sqrt(x^2 + y^2) < xy_range && z > min_z in its own order (stream
 *               compaction, then an exact index over what is left); every source point moved by T.cast<float>() (terms left to right, the rule
 *               of the loop detector's fitness), filtered by the same rule; for the survivors the exact nearest target point by the f32 d2
 *               with d2 <= max_range (on the SQUARED distance).  score = sum / nr (DBL_MAX when nr = 0), n_in = survivors of the source,
 *               inlier ratio = nr / n_in.  THE PROJECT'S RULES: the filter's distance is f32 sqrtf((x*x) + (y*y)), each product and the sum
 *               rounded, compared with xy_range rounded to f32 (the reference's filter() takes floats); both comparisons strict; a point that is
 *               not finite never survives; f64 sums per 256 consecutive source points and then over those records in order; ties to the
 *               smaller index.
 *   align_pairs FAST_VGICP for n arbitrary (target, source) pairs of bank frames in ONE set of rounds: the Gaussian voxels of every distinct
 *               target are built once by the bank's engine and copied into a pool that lives for the call; the per-point arithmetic, the LM
 *               step, the table workgroup -> (slot, first point) and the batch rules are lio_loop_align_candidates': a pair's numbers are
 *               bit-identical to that call on its target alone, whatever its place and neighbours.
 *   accumulate  OM:186-194: the best frame's points, then each neighbour's in the order given (the caller passes rising id: std::set order) moved
 *               by best.pose^-1 * neighbour.pose in f64 (inverse R^T, -(R^T t); every sum of three products left to right) with the Matrix4d rule
 *               of lio_cloud_append_* (f64 per point, terms left to right, cast to f32); then the regularised k-NN covariances of the merged
 *               cloud (the path of lio_gicp_set_target) on an engine sized max_accum_points.  LIO_E_CAPACITY beyond that size.
 *   detect      one detect() call (OM:63-110, 147-211) over a fragment of new frames with poses and connections frozen: candidates per new
 *               frame; the gate for every (new, candidate) pair with guess = (new^-1 * candidate).cast<float>() -- no renormalisation and no
 *               guess(2,3) = 0, unlike the loop detector's guess -- at gate_max_range, pairs with ratio < fitness_inlier_thresh dropped; ONE
 *               align_pairs over all surviving pairs of the fragment; getFitnessScore(fitness_score_max_range) of the converged pairs (PCL's
 *               ungated score, the loop detector's kernel); per new frame a candidate replaces the best unless score > best_score (an equal
 *               score takes the LATER one; no 2 x threshold gate); then per new frame with a best: accumulate, FAST_GICP (target = the
 *               accumulated cloud, source = the new frame, guess = Isometry3f(relative_pose).inverse() in f32 as R^T, -(R^T t), max
 *               correspondence distance fine_max_corr_dist, translation epsilon fine_translation_epsilon = 0.001 (OM:60)); not converged: no
 *               overlap; score = gate(accumulated, new, relative_pose, fitness_score_max_range).score; score > fitness_score_thresh: no overlap.
 * DEVIATIONS.  (1) OM:189 looks a neighbour of the best frame up with std::map::operator[]: a neighbour that is not a frame of the reference map
 * (a new-map frame linked by an earlier fragment's overlap edge) silently becomes index 0 and frame 0 enters the target.  Such a neighbour is
 * SKIPPED here.  (2), (3) inherited from lio_loop_*: the coarse matcher is the non-CUDA branch (FAST_VGICP) and setMaxProcessTime does not
 * apply; an alignment whose H is zero ends NOT converged (ldlt_solve6).  (4) the reference's accumulated target has no size limit; in detect a
 * best frame whose neighbourhood exceeds max_accum_points keeps the neighbours that fit, in std::set order, and the report counts the rest (the
 * stage door lio_overlap_accumulate returns LIO_E_CAPACITY instead).
 * ------------------------------------------------------------------------------------------------------------- */
typedef struct lio_overlap lio_overlap;
typedef struct lio_overlap_params {
    double distance_thresh;            /* 30 (OM:46) */
    int32_t candidate_link_dist;       /* 10 */
    int32_t max_candidate_num;         /* 3 */
    int32_t knn;                       /* 10 (OM:120) */
    float min_z;                       /* 0.5f (OM:227) */
    double fitness_score_max_range;    /* 25, compared with a squared distance */
    double fitness_score_thresh;       /* 1.5 */
    double fitness_inlier_thresh;      /* 0.2 */
    double gate_max_range;             /* 1.0 (OM:160) */
    double xy_range;                   /* 100 (OM:226) */
    double fine_max_corr_dist;         /* 0.5 (OM:59) */
    double fine_translation_epsilon;   /* 0.001 (OM:60); not the loop detector's 0.01 */
    uint32_t max_accum_points;         /* 8 x the bank's max_points */
    uint32_t pad;
} lio_overlap_params;
typedef struct lio_overlap_edge {
    int32_t key1, key2;          /* bank ids: the best frame of the reference map; the new frame */
    float relative_pose[16];     /* getFinalTransformation of the fine matcher, row-major: key2's frame -> key1's frame */
    double score;                /* the gated fitness of the fine result */
    double information[36];      /* lio_loop_information_matrix(score) */
} lio_overlap_edge;
#define LIO_OVERLAP_FOUND 0
#define LIO_OVERLAP_NO_CANDIDATE 1
#define LIO_OVERLAP_GATE 2                /* every candidate's inlier ratio < fitness_inlier_thresh */
#define LIO_OVERLAP_COARSE 3              /* no candidate that passed the gate converged */
#define LIO_OVERLAP_FINE_NOT_CONVERGED 4
#define LIO_OVERLAP_FINE_SCORE 5          /* fine score > fitness_score_thresh */
#define LIO_OVERLAP_ACCUM (-1)            /* lio_overlap_gate_batch's target_id for the cloud of the last lio_overlap_accumulate */
typedef struct lio_overlap_report {
    int32_t new_id;              /* bank id of the new frame */
    int32_t n_candidates;
    int32_t best;                /* index into the candidate list; -1: none */
    int32_t fine_converged, fine_iterations;
    int32_t reason;              /* LIO_OVERLAP_* */
    uint32_t n_accum;            /* points of the fine target; 0: not built */
    int32_t n_neighbours_skipped;/* neighbours of the best frame that are not frames of the reference map (deviation 1) */
    double best_score;           /* coarse; DBL_MAX: none */
    double fine_score;           /* DBL_MAX: not run or nr = 0 */
    int32_t n_neighbours_dropped;/* neighbours of the best frame left out because the target would exceed max_accum_points (deviation 4) */
    int32_t pad;
} lio_overlap_report;
typedef struct lio_overlap_times {
    double candidates_us;        /* host time of the candidate search (wall clock) */
    double gate_us, targets_us, coarse_us, fitness_us, accumulate_us, fine_us; /* HIP events; targets = voxel builds + pool copies */
    int32_t coarse_rounds, n_pairs, n_targets, pad;
} lio_overlap_times;
/* the defaults; bank may be NULL (max_accum_points = 8 x 65536) */
void lio_overlap_default_params(lio_loop* bank, lio_overlap_params*);
/* host only.  get_connection_count over the undirected edges (from[k], to[k]) */
int lio_overlap_connection_count(const int32_t* from, const int32_t* to, uint32_t n_edges, int32_t source, int32_t target, int32_t max_count);
/* host only.  find_candidates over n key frames (positions n x 3 f64, key-frame ids) for a new frame: indices into the n frames in the order
 * they were accepted; the count, or -(count) when cap is too small.  params NULL = the defaults */
int lio_overlap_find_candidates(const double* pos_xyz, const int32_t* ids, uint32_t n, const int32_t* edge_from, const int32_t* edge_to, uint32_t n_edges,
                                int32_t new_id, const double new_xyz[3], const lio_overlap_params* params, int32_t* out_idx, uint32_t cap);
/* NULL without a device or with bad parameters.  params NULL = the defaults */
lio_overlap* lio_overlap_create(lio_loop* bank, const lio_overlap_params* params);
void lio_overlap_destroy(lio_overlap*);
/* stage door: the gate of n bank frames source_ids[] moved by T16 (n x 16 f64, cast to f32) against bank frame target_id (or LIO_OVERLAP_ACCUM).
 * Per pair: score, nr, n_in (any may be NULL) */
int lio_overlap_gate_batch(lio_overlap*, int target_id, const int32_t* source_ids, uint32_t n, const double* T16, double max_range, double* score, uint32_t* nr,
                           uint32_t* n_in);
/* stage door: FAST_VGICP of n (target, source) pairs of bank frames from guesses (n x 16 f64, used as given) in one set of rounds */
int lio_overlap_align_pairs(lio_overlap*, const int32_t* target_ids, const int32_t* source_ids, uint32_t n, const double* guesses, double* out_T,
                            int32_t* iterations, int32_t* converged);
/* stage door: the fine target of best_id and its neighbours (bank ids, in the order given); the number of points, LIO_E_CAPACITY beyond
 * max_accum_points */
int lio_overlap_accumulate(lio_overlap*, int best_id, const int32_t* neighbour_ids, uint32_t n);
/* the accumulated cloud and its covariances (xx, xy, xz, yy, yz, zz) in the cloud's order; the count, or -(count) when cap is too small */
int lio_overlap_download_accum(lio_overlap*, float* xyzi, double* cov6, uint32_t cap);
/* one detect() call.  ref_ids / new_ids: bank ids of the reference map's and the fragment's frames; ref_kf / new_kf: their key-frame ids as
 * the edges name them (NULL: the bank ids).  The overlaps into out (bank ids); the count, or -(count) when cap is too small */
int lio_overlap_detect(lio_overlap*, const int32_t* ref_ids, const int32_t* ref_kf, uint32_t n_ref, const int32_t* new_ids, const int32_t* new_kf, uint32_t n_new,
                       const int32_t* edge_from, const int32_t* edge_to, uint32_t n_edges, lio_overlap_edge* out, uint32_t cap);
/* of new frame k (0 .. n_new) of the last detect; per candidate (arrays of cap entries, any may be NULL): bank id, gate inlier ratio, converged
 * (0 also where the gate refused), iterations, coarse score (DBL_MAX where not taken).  The number of candidates, or -(number) */
int lio_overlap_last_report(lio_overlap*, uint32_t k, lio_overlap_report* report, int32_t* candidate_ids, double* gate_ratio, int32_t* converged, int32_t* iterations,
                            double* scores, uint32_t cap);
/* stage times of the last detect (summed over its frames), or of the last stage-door call for its own stage */
int lio_overlap_last_times(lio_overlap*, lio_overlap_times*);

/* -------------------------------------------------------------------------------------------------------------
 * The Scan Context bank (csrc/scancontext.hip): SCManager of the relocalisation (slam/common/Scancontext/Scancontext.cpp, "SC") with the
 * descriptors of the map's key frames resident in HBM, KeyFrame::computeDescriptor (slam/localization/src/keyframe.cpp:163-168) for many
 * frames in one set of launches, and GlobalLocalization::globalSearch (slam/localization/src/global_localization.cpp:387-413).  A descriptor
 * is 20 rings x 60 sectors of f64, row-major (ring, sector).  THE RULES, restated in numpy by tests/sc_cases.py:
 *   points      a point with a coordinate that is not finite is dropped and counted (lio_sc_last_dropped); the intensity is not read
 *   shift       x' = f32(f64(x) + dx), y' = f32(f64(y) + dy), z' = f32(f64(z) + 0.5) (SC:172-174, LIDAR_HEIGHT)
 *   ring        range = sqrtf(x'*x' + y'*y') in f32; the point is dropped when f64(range) > 80; ring = clamp(ceil(f64(range) / 80 * 20), 1, 20)
 *   sector      theta follows xy2theta's four branches (SC:21-36) with the quotient y'/x' (or its mirrored forms) in f32 as the reference
 *               forms it; the arctangent of that quotient is taken in F64, scaled by 180 / pi in f64, combined with the branch's 180 or 360 in
 *               f64 and rounded ONCE to f32; sector = clamp(ceil(f64(theta) / 360 * 60), 1, 60), and a theta that is not a number (the origin's
 *               0 / 0) goes to sector 1.  DEVIATION: the reference calls atanf, whose last bit differs between libraries; this rule moves a
 *               point only when it lies within an f32 ulp of a sector edge, and makes the device, numpy and glibc agree
 *   bins        a bin starts at -1000 and takes z' when bin < z'; bins still at -1000 become 0 (SC:164-196).  The result is a maximum: it
 *               depends neither on the order of the points nor on how the device cuts a cloud into slices
 *   keys        ring key r = f32((sum over the 60 columns, in column order, in f64) / 60); sector key c = (sum over the 20 rows, in row order) /
 *               20 in f64; column norm c = sqrt(sum of squares in row order).  (Eigen adds in another order: a few ulp.)
 *   ring-key distance   f32, nanoflann's L2_Adaptor::evalMetric (Scancontext/nanoflann.hpp:383-408): five groups of four,
 *               result += ((d0*d0 + d1*d1) + d2*d2) + d3*d3 with d = query - frame.  The min(10, active frames) smallest are the candidates, in
 *               rising distance; equal distances go to the smaller id
 *   distance    distanceBtnScanContext (SC:124-156).  fastAlignUsingVkey: for shift s = 0..59 the norm sqrt(sum over j, in column order, of
 *               (key1[j] - key2[(j - s) mod 60])^2); the smallest by strict < from 10000000, the first shift wins.  The search radius is
 *               round(0.5 * 0.1 * 60) = 3: the shift and its three neighbours on either side mod 60, tried in RISING order of the shift, strict <
 *               from 10000000.  distDirectSC under shift s compares column j of the first with column (j - s) mod 60 of the second: a pair with a
 *               zero norm on either side is skipped, otherwise cos = (dot in row order) / (norm1 * norm2); the result is 1 - (sum of cos in
 *               column order) / count; a count of 0 gives NaN, which wins no <: two descriptors without a common column give {10000000, 0}
 *   yaw         f32(f64(f32(shift * 6.0)) * pi / 180) (SC:322, lio_sc_shift_to_yaw)
 *   search      detectClosestMatch (SC:262-326) scores the candidates in rising ring-key distance and keeps the first of equal scores; its id
 *               is -1 when the score is not below dist_thres; an empty search set gives {-1, yaw 0, score 1}.  globalSearch describes the cloud
 *               under the nine shifts {0,0} {-4,0} {4,0} {0,-4} {0,4} {-4,-4} {-4,4} {4,-4} {4,4}, in that order, and keeps the best by strict <
 * NULL from lio_sc_create without a device: there is no CPU path.  No floating-point atomics; no workgroup waits for another. */
#define LIO_SC_RINGS 20
#define LIO_SC_SECTORS 60
#define LIO_SC_CANDIDATES 10
#define LIO_SC_MAX_SHIFTS 9
typedef struct lio_sc lio_sc;
/* a bank of at most max_frames descriptors; a call stages at most max_points_per_call points (the largest frame, the largest query cloud) */
lio_sc* lio_sc_create(int device, uint32_t max_frames, uint32_t max_points_per_call);
void lio_sc_destroy(lio_sc*);
int lio_sc_reset(lio_sc*);      /* an empty bank, every later frame active */
int lio_sc_num_frames(lio_sc*);
/* the map load: frame k is points [offsets[k], offsets[k + 1]) of xyzi (n x 4 f32), described under the shift (0, 0); as many whole frames as
 * fit max_points_per_call go into one set of launches.  The id of the first frame (ids rise by one); LIO_E_CAPACITY beyond max_frames or for
 * a frame larger than max_points_per_call, with the bank as it was */
int lio_sc_add_frames_host(lio_sc*, const float* xyzi, const uint64_t* offsets, uint32_t n_frames);
/* a frame's descriptor (1200 f64), ring key (20 f32) and sector key (60 f64); any may be NULL */
int lio_sc_download_frame(lio_sc*, int id, double* desc, float* ringkey, double* sectorkey);
/* stage door: makeScancontext(cloud, dx, dy) of one cloud under n_shifts (1..9) shifts (dx, dy pairs) in one set of launches; per shift the
 * descriptor, ring key and sector key (any may be NULL) */
int lio_sc_describe_host(lio_sc*, const float* xyzi, uint32_t n, const double* shifts_xy, uint32_t n_shifts, double* desc, float* ringkey, double* sectorkey);
/* the frames a search looks at (mSearchIdxMap of setInitPoseRange, the range filter applied by the caller): n distinct ids; n = 0 is the empty
 * set; n < 0 is every frame of the bank, later ones included (the state after create and reset) */
int lio_sc_set_active(lio_sc*, const int32_t* ids, int32_t n);
/* stage door: distanceBtnScanContext(desc_a[k], desc_b[k]) for n_pairs pairs of descriptors (1200 f64 each) */
int lio_sc_distance(lio_sc*, const double* desc_a, const double* desc_b, uint32_t n_pairs, double* dist, int32_t* shift);
/* per query (descriptor and ring key) the candidates among the active frames in rising ring-key distance, with the distance and shift of each:
 * detectCandidateMatch (SC:328-361) without its threshold.  10 entries per query; places past n_cand[q] = min(10, active) hold id -1, NaN, -1.
 * Any output may be NULL */
int lio_sc_search(lio_sc*, const double* desc, const float* ringkey, uint32_t n_queries, int32_t* cand_ids, double* cand_dist, int32_t* cand_shift, int32_t* n_cand);
/* globalSearch of a cloud: the matched frame's id (-1: the best score is not below dist_thres; 0.30 with point clouds alone), the yaw, the
 * score and the column shift behind the yaw (any may be NULL) */
int lio_sc_global_search_host(lio_sc*, const float* xyzi, uint32_t n, double dist_thres, int32_t* match_id, float* yaw, double* score, int32_t* shift);
/* the key frames' positions (n_frames x 3 f32: the translations of their poses rounded to f32), row k = bank id k, resident beside the
 * descriptors; what localSearch's kd-tree (mGraphKDTree) holds.  n_frames must be the bank's number of frames when a local search runs */
int lio_sc_set_positions(lio_sc*, const float* xyz, uint32_t n_frames);
/* GlobalLocalization::localSearch (global_localization.cpp:350-385), the INS-aided start.  The cloud is described once under the shift (0, 0).
 *   nearest     the min(10, F) frames nearest to (f32(ins_x), f32(ins_y), 0) among ALL F frames of the bank (the active set is not read: the
 *               reference's kd-tree holds every key frame).  The query's z is 0 while a frame keeps its own z: the reference's quirk, kept.
 *               f32 with d = frame - query: d2 = ((dx*dx) + dy*dy) + dz*dz.  In rising (d2, id): equal distances go to the SMALLER ID.  (PCL's
 *               kd-tree leaves the order of ties undefined; this is the project's rule.)  A d2 that is not a number sorts after every number.
 *   distances   distanceBtnScanContext of the cloud's descriptor to each of those frames, the bank's rows read by id on the device
 *   walk        on the host, in that order, from match = -1 and min_dist = 1.0: without a match yet, f64(d2) > precision^2 ends the search
 *               with -1 ("far from the map"); with one, f64(d2) > precision^2 / 10 ends the walk; otherwise the frame's distance is read and
 *               wins by strict <.  No dist_thres applies.  n_examined = the distances the walk read.  An empty bank answers -1, 0 read.
 * match_id -1 comes with yaw 0 and score 1.0.  ins_xyz[2] is not read.  LIO_E_STATE when the positions do not cover the bank;
 * LIO_E_INVALID when ins_xyz[0], ins_xyz[1] or the precision is not finite (both gates would be false for them).
 * Any output may be NULL */
int lio_sc_local_search(lio_sc*, const float* xyzi, uint32_t n, const double ins_xyz[3], double precision, int32_t* match_id, float* yaw, double* score,
                        int32_t* n_examined);
/* what the last local search walked over: the nearest frames in rising (d2, id) with d2, Scan Context distance and column shift of each (10
 * entries each, any may be NULL; places past the returned count min(10, F) hold -1, inf, NaN, -1), and the shift of the match (0 without one) */
int lio_sc_last_local(lio_sc*, int32_t* ids, float* d2, double* dist, int32_t* shift, int32_t* match_shift);
/* host only: the yaw of a column shift */
float lio_sc_shift_to_yaw(int32_t shift);
/* points the last add_frames / describe / global_search call dropped because a coordinate was not finite */
int lio_sc_last_dropped(lio_sc*, uint64_t* n_nonfinite);
/* device time (HIP events) of the last call's stages in us: upload + describe, ring-key search, distances (any may be NULL) */
int lio_sc_last_times(lio_sc*, double* describe_us, double* ringkey_us, double* distance_us);

/* -------------------------------------------------------------------------------------------------------------
 * The pose graph on the device (csrc/graph.hip): what hdl_graph_slam's GraphSLAM does with g2o for SE3 pose nodes and EdgeSE3 edges
 * (graph_slam.cpp:344-375, solver "lm_var").  g2o is not in the reference tree: THE RULES BELOW ARE RESTATED FROM g2o'S PUBLISHED SOURCE
 * (types/slam3d/isometry3d_mappings, edge_se3, core/robust_kernel_impl, core/optimization_algorithm_levenberg) and are pinned to an f64 numpy
 * restatement (tests/graph_cases.py, tests/graph_prior_cases.py, tests/graph_moment_cases.py), not to a compiled reference.  Out of scope: the
 * reference's EdgeSE3PriorVec (its only producer, imu_callback, returns at once: hdl_graph_slam_nodelet.cpp:462-463).  NULL from
 * lio_graph_create without a device: there is no CPU fallback.
 *   state       a node is an f64 translation, a unit quaternion and a fixed flag; an edge is from, to, a measurement M (given as a row-major
 *               4 x 4, kept as translation + quaternion), an f64 6 x 6 information matrix, a kernel and its delta.  Ids count from 0 in creation
 *               order and are never reused; a removed edge takes no part.
 *   error       e = toVectorMQT(M^-1 X_from^-1 X_to): the translation, then x, y, z of the normalised quaternion, its sign chosen so that w >= 0.
 *   update      X <- X fromVectorMQT(d): t += R d[0:3]; q <- q (d[3:6], w), w = sqrt(1 - |d_q|^2); the identity rotation when 1 - |d_q|^2 < 0.
 *               THE PROJECT'S RULE: the rotation is kept as a quaternion and renormalised after every update (g2o keeps a matrix and
 *               orthogonalises it every 1000 updates).
 *   cost        chi2_e = e^T Omega e.  Huber: sqrt(chi2_e) <= delta: rho = chi2_e, rho' = 1; otherwise rho = 2 delta sqrt(chi2_e) - delta^2,
 *               rho' = delta / sqrt(chi2_e).  The quadratic form uses rho' Omega with no second-order term: b += -J^T (rho' Omega) e,
 *               H += J^T (rho' Omega) J.  The graph's chi2 is the sum of rho over the live edges.
 *   Jacobians   analytic: the derivative of e with respect to the two nodes' d at 0.
 *   priors      a prior is a unary edge of three rows on one node (hdl_graph_slam's EdgeSE3PriorXYZ, EdgeSE3PriorQuat, EdgeSE3Plane; the plane
 *               vertex of the last is always fixed in the reference, :563, so the edge carries its world plane and there is no plane vertex).
 *               It takes the next id of the same counter as the binary edges (graph_slam.cpp's max_edge_id++), ids are never reused,
 *               lio_graph_remove_edge removes either kind, a prior counts towards min_edges and gives its node a live edge: a free node whose only
 *               live edges are priors is active.  A prior on a fixed node adds its rho to chi2 and nothing to H or b.  With R, t, q = (v, w) of
 *               the node:
 *                 XYZ    (edge_se3_priorxyz.hpp:39-44)  e = t - m;  J = [R, 0]
 *                 QUAT   (edge_se3_priorquat.hpp:39-55) the measurement is normalised on entry (THE PROJECT'S RULE) and flipped so that w_m >= 0;
 *                        s = -1 if m . q < 0 else +1;  e = s v - v_m;  J = [0, s (w I + [v]x)]
 *                 PLANE  (edge_se3_plane.hpp:40-47, g2o's Plane3D) the world plane (n, d) and the measurement (n_m, d_m) are each divided by
 *                        the norm of their normal on entry;  n_l = R^T n, d_l = d + t . n;  az(x) = atan2(x_y, x_x), el(x) = atan2(x_z,
 *                        hypot(x_x, x_y));  A = Rz(az(n_m)) Ry(-el(n_m)), u = A^T n_l;  e = (az(u), el(u), d_m - d_l).  With r^2 = u_x^2 + u_y^2
 *                        and D = 2 A^T [n_l]x: row 0 of J is [0, (-u_y, u_x, 0) / r^2 D], row 1 is [0, (-u_x u_z / r, -u_y u_z / r, r) D], row 2 is
 *                        [-n_l^T, 0].  THE PROJECT'S RULE: rows 0 and 1 are zero when r^2 == 0.
 *               g2o differentiates these edges numerically (central differences, 1e-9); THE ANALYTIC JACOBIANS ARE THE PROJECT'S RULE.
 *               chi2_e = e^T Omega e with a symmetric 3 x 3 Omega, refused by the same test as the 6 x 6.
 *   DCS2        (robust_kernel_dcs2.hpp, either kind of edge) phi = delta, s = 2 phi / (phi + chi2_e).  s >= 1: rho = chi2_e, rho' = 1; otherwise
 *               rho = s^2 chi2_e, rho' = 4 phi^2 (phi - chi2_e) / (phi + chi2_e)^3.  rho' is negative for chi2_e > phi and is used as it is (g2o
 *               does the same); a diagonal block that stops being positive definite fails the trial (CHOLMOD would fail there too).
 *   outliers    THE PROJECT'S NAME for the first stage of robust_graph_optimize (:1004-1038), lio_graph_remove_gnss_outliers: every live XYZ prior
 *               gets DCS2 with delta = max_err^2 Omega(0,0); optimise; every XYZ prior with 2 phi / (phi + chi2_e) < 0.1 (the unrobustified
 *               chi2_e) is removed; optimise again.  The priors that stay keep DCS2.
 *   moment      THE PROJECT'S NAME for the second stage of robust_graph_optimize in mode `mapping` (:1037-1081), lio_graph_estimate_gnss_moment: the
 *               constant offset m between the GNSS antenna and the lidar frame, one shared VertexPointXYZ (3 DoF, updated additively: m <- m + d_m).
 *               While the stage is open every live XYZ prior is an EdgeSE3GNSS (edge_se3_gnss.hpp:39-45) on its node (t, R) and m:
 *                 e = t - (z + R m);  d e / d d = [R | 2 R [m]x] (3 x 6, under X <- X fromVectorMQT(d));  d e / d m = -R
 *               (ANALYTIC, THE PROJECT'S RULE: g2o differentiates this edge numerically).  SIGN: with fixes z = t + R l, l the antenna's place in
 *               the lidar frame, the stage finds m = -l, not l; the moved measurements z' = z + R m = t are the lidar's own positions.  This is
 *               the reference's convention and is not a mistake to be mended.  The stage, statement for statement: (1) m = 0 with an EdgeXYZPrior
 *               at 0 of information diag(1/2000, 1/2000, 1/200), e_m = m, no kernel; (2) every live XYZ prior becomes a moment edge with the same
 *               node, measurement and information and DCS2 with phi = max_err^2 Omega(0,0), max_err = 1.0; (3) optimize(1024); (4) every moment
 *               edge becomes an XYZ prior again with z' = z + R_node m, the same information and DCS2; (5) the moment and its prior are removed.
 *               THE PROJECT'S RULE: the reference deletes and re-creates the edges, so every GNSS prior gets a new id and the counter advances by
 *               2 n; here a prior keeps its id and changes its measurement in place (ids stay stable for a caller that shows them, as for
 *               lio_graph_remove_node, and no dead placeholder is left).  The moment vertex's id (1000000) is never visible.
 *               The system with the moment present has 6 Na + 3 unknowns: per moment edge on an active node a 6 x 3 coupling block
 *               J^T (rho' Omega) J_m, and J_m^T (rho' Omega) J_m and -J_m^T (rho' Omega) e into the border's 3 x 3 and b_m, to which the moment's
 *               prior adds Omega_m and -Omega_m m.  A moment edge on a fixed node contributes to the 3 x 3, b_m and chi2 only.  LM: lambda_0 takes
 *               the largest |diag H| over the border's three entries too, d^T (lambda d + b) covers them, a rejected trial restores m with the
 *               poses, the moment's prior is one live edge for min_edges and its m^T Omega_m m is part of chi2 (added after the per-256 records).
 *               The solve's preconditioner has the damped 3 x 3's inverse as one more block; with no active node the cap on its iterations is 3
 *               (THE PROJECT'S RULE, as the solve is).
 *               Sums: a node's coupling block, the 3 x 3 and b_m are summed in rising edge id; the border rows' sum over the nodes is folded
 *               in the solve's fixed order.
 *   active set  a fixed node contributes no unknowns; a node with no live edge is left out of the solve and keeps its estimate.
 *   LM          OptimizationAlgorithmLevenberg: lambda_0 = 1e-5 max diag(H), nu = 2.  A trial solves (H + lambda I) d = b, applies the update and
 *               re-evaluates chi2; rho = (chi2_old - chi2_new) / (d^T (lambda d + b) + 1e-3).  Accepted (rho > 0, chi2_new finite): lambda *=
 *               max(1/3, min(2/3, 1 - (2 rho - 1)^3)), nu = 2.  Rejected: the estimates are restored, lambda *= nu, nu *= 2.  An iteration takes
 *               trials while rho < 0, at most 10.  The optimisation stops after max_iterations, after an iteration whose tenth trial was
 *               reached, on rho = 0, or on a non-finite lambda; every iteration begun counts in the return value.  THE PROJECT'S OWN stop rule,
 *               off by default: chi2_rel_stop > 0 stops after an accepted step that lowers chi2 by no more than that fraction of it.
 *   solve       THE PROJECT'S RULE: g2o factorises (CHOLMOD); this runs conjugate gradients in f64, preconditioned by the inverse of every
 *               node's damped 6 x 6 diagonal block, until |r| <= cg_epsilon |b| or cg_max_iterations (0: 12 x active nodes).  An inexact step is
 *               still safe: the rho test judges it.  The iterations and the final relative residual are in the report.
 *   sums        every block of H (one diagonal block per active node, one off-diagonal block per distinct pair) and of b is the sum of its
 *               edges' contributions in rising edge id, binary and unary interleaved by id; chi2 is summed per 256 consecutive edge ids (of
 *               either kind) and then over those records in order; the
 *               dot products of the solve are folded in a fixed order.  No floating-point atomics: two runs give the same bits.
 * ------------------------------------------------------------------------------------------------------------- */
typedef struct lio_graph lio_graph;
#define LIO_GRAPH_KERNEL_NONE 0
#define LIO_GRAPH_KERNEL_HUBER 1
#define LIO_GRAPH_KERNEL_DCS2 2
#define LIO_GRAPH_PRIOR_XYZ 0
#define LIO_GRAPH_PRIOR_QUAT 1
#define LIO_GRAPH_PRIOR_PLANE 2
#define LIO_GRAPH_STOP_MAX_ITERATIONS 1
#define LIO_GRAPH_STOP_TRIALS 2          /* the tenth trial of an iteration was reached */
#define LIO_GRAPH_STOP_RHO_ZERO 3
#define LIO_GRAPH_STOP_LAMBDA 4          /* lambda is no longer finite */
#define LIO_GRAPH_STOP_CHI2_REL 5        /* chi2_rel_stop */
typedef struct lio_graph_params {
    double cg_epsilon;          /* 1e-10 */
    double chi2_rel_stop;       /* 0: off */
    int32_t min_edges;          /* 10 (graph_slam.cpp:346) */
    int32_t cg_max_iterations;  /* 0: 12 x the number of active nodes */
} lio_graph_params;
typedef struct lio_graph_report {
    int32_t iterations;           /* LM iterations run */
    int32_t stop_reason;          /* LIO_GRAPH_STOP_*; 0: nothing to do */
    int32_t trials, accepted;     /* trials in all; those accepted */
    int32_t n_active, n_live_edges;
    int32_t cg_iterations;        /* of the last solve */
    int32_t cg_iterations_total;
    double chi2_initial, chi2_final, lambda;
    double cg_residual;           /* |r| / |b| at the end of the last solve */
} lio_graph_report;
void lio_graph_default_params(lio_graph_params*);
/* params NULL = the defaults */
lio_graph* lio_graph_create(int device, const lio_graph_params* params);
void lio_graph_destroy(lio_graph*);
/* no nodes, no edges; memory is kept */
int lio_graph_reset(lio_graph*);
/* poses are row-major 4 x 4 f64; the rotation goes through Eigen's matrix -> quaternion conversion and is normalised.  The id */
int lio_graph_add_node(lio_graph*, const double pose16[16]);
int lio_graph_set_fixed(lio_graph*, int id, int flag);
int lio_graph_set_estimate(lio_graph*, int id, const double pose16[16]);
int lio_graph_num_nodes(lio_graph*);
/* the fixed flags of all nodes; the count, or -(count) when cap is too small */
int lio_graph_get_fixed(lio_graph*, uint8_t* out, uint32_t cap);
/* the id; LIO_E_INVALID for from == to, an unknown node or kernel, a kernel with delta <= 0, or an information matrix that is not finite or not
 * symmetric to 1e-9 of its largest entry */
int lio_graph_add_edge(lio_graph*, int from, int to, const double M16[16], const double info36[36], int kernel, double delta);
int lio_graph_remove_edge(lio_graph*, int id);
/* graph_del_vertex / GraphSLAM::del_se3_node (hdl_graph_slam_nodelet.cpp:868-891, graph_slam.cpp:154-156: g2o's removeVertex, which removes every
 * edge incident to the vertex as well): the node is marked removed and every live edge and prior on it is removed as lio_graph_remove_edge
 * removes it.  Ids are g2o ids and stay: no other node or edge is renumbered, the id is never handed out again, lio_graph_num_nodes goes on
 * counting the slot.  Afterwards the id is unknown: lio_graph_add_edge, _add_prior, _set_fixed, _set_estimate and a second _remove_node answer
 * LIO_E_INVALID.  A removed node is never active (no row, no block, no preconditioner entry); lio_graph_estimates leaves its row as it last
 * was, lio_graph_get_fixed reports 0 for it.  When the only fixed node is removed the next optimisation runs as the graph always has without a
 * fixed node: every connected node is active, nothing but the LM damping holds the gauge, chi2 still falls and the whole graph may drift rigidly */
int lio_graph_remove_node(lio_graph*, int id);
/* 1 for a live node, 0 for a removed one, all slots; the count, or -(count) when cap is too small (as lio_graph_get_fixed) */
int lio_graph_node_live(lio_graph*, uint8_t* out, uint32_t cap);
/* the live binary edges in rising id as they were added -- what graph_save (hdl_graph_slam_nodelet.cpp:1088-1110) hands to g2o's writer: id, ends,
 * the measurement as the row-major 4 x 4 and the 6 x 6 information bit for bit as lio_graph_add_edge received them (the graph keeps a host copy;
 * the device holds the measurement as t + q), the kernel and delta as lio_graph_set_kernel last left them.  Any array may be NULL; the count, or
 * -(count) when cap is too small (as lio_graph_priors, whose counterpart this is) */
int lio_graph_edge_records(lio_graph*, int32_t* id, int32_t* from, int32_t* to, double* M16, double* info36, int32_t* kernel, double* delta, uint32_t cap);
/* a prior on one node: type LIO_GRAPH_PRIOR_*; m4 = x, y, z (XYZ; m4[3] is not read), a quaternion x, y, z, w (QUAT) or a plane n, d in the node's
 * frame (PLANE); plane4 = the world plane of a PLANE prior (NULL otherwise); info9 row-major 3 x 3.  The id; LIO_E_INVALID for an unknown node,
 * type or kernel, a kernel with delta <= 0, a value that is not finite, a zero normal or quaternion, or an information matrix that is not
 * symmetric to 1e-9 of its largest entry */
int lio_graph_add_prior(lio_graph*, int node, int type, const double m4[4], const double* plane4, const double info9[9], int kernel, double delta);
/* the robust kernel of a live edge of either kind */
int lio_graph_set_kernel(lio_graph*, int edge_id, int kernel, double delta);
/* the live priors in rising id, as the graph keeps them (any array may be NULL; m4 and plane4 4 per prior, info9 9); the count, or -(count) when
 * cap is too small */
int lio_graph_priors(lio_graph*, int32_t* id, int32_t* node, int32_t* type, double* m4, double* plane4, double* info9, int32_t* kernel, double* delta, uint32_t cap);
/* the GNSS outlier stage (the rules above, "outliers"): the number of priors removed, their ids into removed_ids (the first cap of them; may be
 * NULL); -1 with nothing touched when fewer than min_edges live edges exist.  report (may be NULL) is of the second optimisation */
int lio_graph_remove_gnss_outliers(lio_graph*, double max_distance_error, int max_iterations, int32_t* removed_ids, uint32_t cap, lio_graph_report* report);
/* the GNSS moment stage (the rules above, "moment"): the number of XYZ priors re-anchored, the moment into moment3 (may be NULL).  prior_info9 =
 * the information of the moment's prior at 0 (NULL: the reference's diag(1/2000, 1/2000, 1/200)).  0 with nothing touched when no live XYZ prior
 * exists; LIO_E_STATE with nothing touched when fewer than min_edges live edges exist (the moment's prior counted as one), or between
 * lio_graph_moment_begin and _end.  report (may be NULL) is of the stage's optimisation */
int lio_graph_estimate_gnss_moment(lio_graph*, double max_distance_error, int max_iterations, const double* prior_info9, double moment3[3], lio_graph_report* report);
/* stage doors of the moment stage.  _begin opens it at the moment m0 (NULL: 0) with the prior information info9 (NULL: the reference's) and
 * changes no kernel; until _end, lio_graph_optimize, lio_graph_chi2 and lio_graph_linearize run over the bordered system (every live XYZ prior a
 * moment edge), and lio_graph_add_node / _add_edge / _add_prior / _remove_edge / _remove_node / _reset / _remove_gnss_outliers /
 * _estimate_gnss_moment and a second _begin answer LIO_E_STATE.  _end with apply != 0 moves every live XYZ prior's measurement to z + R_node m
 * and returns their number; with apply == 0 it drops the moment and leaves every prior as it was (0).  _get: the current moment.  _linearize: one
 * linearisation as lio_graph_linearize, and from it b_m, the border's 3 x 3 (row-major) and per node id the 6 x 3 coupling block (row-major, 18
 * per node; zeros for a node that is fixed or carries no moment edge; node_cap in nodes); the number of moment edges.  _get, _end and _linearize
 * answer LIO_E_STATE when no stage is open */
int lio_graph_moment_begin(lio_graph*, const double* m0, const double* info9);
int lio_graph_moment_end(lio_graph*, int apply);
int lio_graph_moment_get(lio_graph*, double m3[3]);
int lio_graph_moment_linearize(lio_graph*, double bm3[3], double Hmm9[9], double* Hpm, uint32_t node_cap);
/* the iterations run; -1 with nothing touched when fewer than min_edges live edges exist (GraphSLAM::optimize); other negative values are
 * LIO_E_* (a NULL handle is LIO_E_INVALID = -1 as well).  report may be NULL */
int lio_graph_optimize(lio_graph*, int max_iterations, lio_graph_report* report);
/* all estimates as row-major 4 x 4 (cap in nodes); the count, or -(count) when cap is too small */
int lio_graph_estimates(lio_graph*, double* out16, uint32_t cap);
/* the live edges in rising id (any array may be NULL); a prior has from = its node and to = -1; the count, or -(count) when cap is too small */
int lio_graph_edges(lio_graph*, int32_t* from, int32_t* to, int32_t* id, uint32_t cap);
int lio_graph_chi2(lio_graph*, double* chi2);
/* stage door: one linearisation at the current estimate, no step taken.  Per edge id (removed edges: zeros; a prior's error in the first three
 * of its six slots) the error, chi2_e and rho'; per node
 * id (fixed or unconnected nodes: zeros) b and the diagonal block of H.  Any output may be NULL; the number of edge ids, LIO_E_CAPACITY when a
 * cap is too small */
int lio_graph_linearize(lio_graph*, double* errors, double* chi2, double* rho1, uint32_t edge_cap, double* b, double* Hdiag, uint32_t node_cap);
/* device time (HIP events) of the last lio_graph_optimize in us: linearise, assemble, solve, update (update + chi2 + the LM bookkeeping) */
int lio_graph_last_times(lio_graph*, double* linearize_us, double* assemble_us, double* solve_us, double* update_us);
/* host only (no device needed): g2o's fromVectorMQT / toVectorMQT on row-major 4 x 4, and the edge error of three poses */
void lio_se3_from_mqt(const double v6[6], double T16[16]);
void lio_se3_to_mqt(const double T16[16], double v6[6]);
int lio_graph_edge_error(const double Xfrom16[16], const double Xto16[16], const double M16[16], double e6[6]);
/* host only: a prior's error at the pose X; m4 and plane4 as lio_graph_add_prior takes them (normalised here the same way) */
int lio_graph_prior_error(const double X16[16], int type, const double m4[4], const double* plane4, double e3[3]);

/* manifold helpers exposed for known-answer tests (mtk SO3/S2 boxplus/boxminus, SOn.hpp:233-245, S2.hpp:136-167) */
void lio_state_boxplus(const double s26[26], const double d23[23], double out26[26]);
void lio_state_boxminus(const double a26[26], const double b26[26], double d23[23]);

/* -------------------------------------------------------------------------------------------------------------
 * Colour map on the device (csrc/render.hip): MapRender of slam/localization/map_render/ -- map_render.cpp (MR), render_common.h (RC),
 * image_render.hpp's ImageRenderCpu (IR), camera_model.{h,cpp} (CM) -- and the same painter behind graph_utils.cpp:503-622.  PCL, OpenCV and
 * Boost are restated from their published behaviour; where the reference has no order of its own (it iterates hash containers of pointers)
 * the rule is THE PROJECT'S and is marked so.  NULL from lio_render_create without a device: there is no CPU fallback.
 * Constants (RC:10-15): point resolution 0.02, voxel 0.2, their inverses 1.0 / 0.02 and 1.0 / 0.2 in f64, depth 2.0 to 80.0.
 *   gate     (render, MR:197-211) nothing happens while the painter is inactive, nor while the translation of last_pose^-1 pose is shorter
 *            than 0.1 m; last_pose starts as identity (a first frame near the origin is skipped) and is updated BEFORE the ground test.
 *            Then detect_ground (MR:81-134): lio_ground preset 0 (clip 1.5 / 1.5, normals 20 deg, 1024 points, floor 10 deg) with
 *            distance_threshold = 0.2 (MR:101) and the seeded draws of lio_ground; no floor: nothing else happens.  On success the frame IS
 *            REPLACED by the floor inliers (MR:129-132); only they are inserted and painted.  PROJECT: poses are taken as rigid, the inverse
 *            of (R, t) is (R^T, -(R^T t)), every sum of three products left to right in f64.
 *   world    pose (f64) applied to the f32 points and rounded to f32 by the rule of lio_cloud_append_host (MR:215).
 *   insert   (updateMap, MR:165-195) in f64 from the f32 world point: box = round(x * (1 / 0.2)) half away from zero; voxel centre
 *            c = int64((box * 0.2) * (1 / 0.02)) truncating; per axis o = int64(x * (1 / 0.02)) - c + 5; key = ox * 100 + oy * 10 + oz.  A
 *            point is stored only if its voxel does not hold that key yet.  (The key is kept as it is: it is not injective over offsets 0 .. 10,
 *            but x * 5 and x * 50 are exact in f64 for an f32 x, so the offsets of one voxel are ten consecutive values per axis, 0 .. 9 or
 *            1 .. 10, and over those distinct cells never share a key.)  Of several points of
 *            one frame with the same (voxel, key) the one earliest in the input is stored.  Every voxel touched by the frame, by stored
 *            and rejected points alike, is a hit: hits + 1 per rendered frame, before any image is looked at, also without images.
 *            PROJECT: voxels are numbered in order of the input index that created them, points get serial numbers in input order; a
 *            point that is not finite or whose box leaves +-2^20 is dropped.
 *   camera   (CameraModel, ImageRender::setPose, IR:13-38, CM:3-26) K is read as f32 and widened; static_trans = camera_extrinsic *
 *            lidar_static^-1 (setParameter, MR:152-157), ext = static_trans^-1; R_w2c = R_pose R_ext, t_w2c = R_pose t_ext + t_pose; the
 *            camera-from-world map is R = R_w2c^T, t = -(R t_w2c).  PROJECT: pt_cam = R p + t with R as a matrix (the reference goes through
 *            an Eigen quaternion), every sum of three products left to right in f64, no fusion.  project3DPoints (CM:39-47) fails if
 *            z < 0.001; u = x fx / z + cx, v = y fy / z + cy.  point2DAvailable (CM:49-57): u >= 0.005 cols + 1 && ceil(u) < (1 - 0.005) cols,
 *            the same for v with rows.
 *   voxel    (MR:251-297, per image and hit voxel) the centre c * 0.02 must project, be available and have 2.0 < z < 80.0, else the voxel
 *            contributes nothing to this image.  Then every stored point of the voxel (of earlier frames too) is projected; one that does
 *            not project or is not available is skipped.  The bounding box of (u, v) starts at the centre's and grows over the kept points;
 *            max_u - min_u <= 10 && max_v - min_v <= 10 masks the whole voxel for this image.
 *   z-buffer (MR:299-316) pixel (round(u), round(v)) half away from zero; the winner of a pixel is the kept, unmasked point with the smallest
 *            (float)z.  PROJECT: ties go to the smaller serial number (a 64-bit atomicMin over (f32 depth bits, serial)).
 *   window   (checkDepthContinuous, IR:66-90, the f64 variant: the CUDA one narrows u and v to f32 first) for each winner the 9 x 9 cells
 *            ((int)(u + i), (int)(v + j)), i, j = -4 .. 4 (truncation here, where the z-buffer rounds); cells outside the image or without
 *            an owner are skipped; min / max are f32 and start at (float)z; the winner is valid iff max - min <= 2.0.
 *   blend    (update_voxel_rgb, RC:192-217, for every valid winner; images in ascending name order, each finished before the next)
 *            score = (float)(1 - |u - cols / 2| / (cols / 2)) (MR:288); skip if score < 0.1; skip if z > 1.5 m_depth (m_depth f32, starts at
 *            100, compared in f64); if z < m_depth, m_depth = (float)z; rgb[k] = (float)((rgb[k] s1 + c_k s2) / (s1 + s2)) with s1 = m_score
 *            and s2 = score widened to f64 and c = (R, G, B) of the BGR sample; m_score = max(s1, s2).  Tracks and COLMAP are out of scope.
 *   sample   (getSubPixel<cv::Vec3b>(image, v, u), CM's header :22-42, OpenCV's Matx operators) weights (1 - fr)(1 - fc), fr (1 - fc),
 *            (1 - fr) fc, fr fc for (floor, floor), (ceil row, floor col), (floor row, ceil col), (ceil, ceil), ceil = floor + 1; each term
 *            w * pixel per channel rounded to u8 on its own (half to even, saturated), the four added left to right with saturation.  A tap
 *            of weight zero is not read and contributes 0 (the reference reads past the edge of images under 200 px there).  Images are
 *            rows x cols x 3 u8, BGR; imageCvtColor's conversions are out of scope.
 *   export   (getColorMap, MR:327-353) a point is written when its voxel has hits > 2 and its own score >= 0.1; PROJECT: in ascending voxel
 *            number, then serial number; x, y, z as stored, each channel truncated to u8 and packed r << 16 | g << 8 | b, the word
 *            reinterpreted as f32 (pointcloud_to_numpy(PointCloudRGB), py_utils.cpp:118-129).
 * ------------------------------------------------------------------------------------------------------------- */
typedef struct lio_render lio_render;
typedef struct lio_render_image {
    int32_t camera;      /* index into the cameras of lio_render_set_cameras */
    int32_t rows, cols;
    int32_t reserved;
    const uint8_t* bgr;  /* rows x cols x 3, host */
    double pose[16];     /* row-major, the pose at the image's stamp */
} lio_render_image;
#define LIO_RENDER_SKIPPED 0  /* inactive, or moved less than 0.1 m */
#define LIO_RENDER_NO_FLOOR 1 /* the ground test found no floor (last_pose has moved) */
#define LIO_RENDER_DONE 2     /* inserted and painted */
/* the map holds at most max_voxels voxels and max_points points (4 max_points + 8 max_voxels < 2^32) */
lio_render* lio_render_create(int device, uint64_t max_voxels, uint64_t max_points);
void lio_render_destroy(lio_render*);
/* drops the map (MapRender::clear); cameras, the active flag and last_pose stay */
int lio_render_clear(lio_render*);
/* n cameras: names (distinct), intrinsics n x (fx, fy, cx, cy), extrinsics n x 16 row-major, lidar_static 16 or NULL (identity) */
int lio_render_set_cameras(lio_render*, int n, const char* const* names, const double* intrinsics, const double* extrinsics, const double* lidar_static);
int lio_render_set_active(lio_render*, int active);
/* render(pose, frame, images) over n host points (x, y, z, intensity): LIO_RENDER_* or an error.  use_ground = 0 takes the points as they are
 * (no ground test).  At most one image per camera; they are painted in ascending camera name.  Capacity is checked before anything is
 * committed: a frame that does not fit returns LIO_E_CAPACITY and leaves the map unchanged (last_pose has moved). */
int lio_render_frame(lio_render*, const float* xyzi, uint64_t n, const double pose[16], int use_ground, uint32_t seed, const lio_render_image* images,
                     int n_images);
int lio_render_size(lio_render*, uint64_t* n_voxels, uint64_t* n_points);
/* the export above: n x 4 f32; returns n, or -n when cap (points) is too small */
int64_t lio_render_download(lio_render*, float* xyzrgb, uint64_t cap);
/* read-backs for tests, in voxel number / serial number order; any array may be NULL; the count, or -(count) when cap is too small.
 * voxels: box triple, hits, stored points; points: position, voxel number, rgb (f32), m_score, m_depth;
 * last_image: of the last image of the last rendered frame -- depth buffer (-1: no owner), owner serial (-1) and valid flag per pixel */
int64_t lio_render_download_voxels(lio_render*, int32_t* box3, uint32_t* hits, uint32_t* counts, uint64_t cap);
int64_t lio_render_download_points(lio_render*, float* xyz, uint32_t* voxel, float* rgb, float* score, float* depth, uint64_t cap);
int64_t lio_render_download_last_image(lio_render*, float* depth, int32_t* owner, uint8_t* valid, uint64_t cap, int* rows, int* cols);
/* device time (HIP events) of the last rendered frame: insert chain, all images, finish + read-back */
int lio_render_last_times(lio_render*, double* insert_us, double* image_us, double* finish_us);

/* ---------------------------------------------------------------------------------------------------------------
 * Geodesy and the RTK track: the GNSS side of mapping mode.  Host code, f64, no device (csrc/geodesy.cpp).
 * Reference files: UP = sensor_driver/common_lib/cpp_utils/UTMProjector.cpp, SU = slam/common/slam_utils.cpp,
 * RK = slam/mapping/rtkm/src/rtkm.cpp, HG = slam/backend/hdl_graph_slam/apps/hdl_graph_slam_nodelet.cpp.  Every function restates its
 * original statement for statement, in the original's order of evaluation; the library is built without contraction.
 *   lio_utm     UTMProjector.  forward = FromGlobalToLocal (UP:13-55), inverse = FromLocalToGlobal (UP:57-109), longitude0 = GetLongitude0
 *               (UP:111-117).  Quirks kept: zone width and zone number are ints (UTMProjector.h:13-14); the zone number is fixed by the first
 *               call (forward: floor(longitude / width); inverse: floor(x / 1000000) - 1 with the width hard-coded to 6) and sticks -- "unset"
 *               is `zone < 0`, so a zone west of Greenwich is derived again by every call; width / 2 is an integer division;
 *               f = 1 / 298.257222101; false easting 1000000 (zone + 1) + 500000; scale 0.9996 about 500000.  lio_utm_zone is the zone
 *               number, -1 on a fresh handle; longitude0 of a fresh handle is -1 * width + width / 2 as in the reference (which warns).
 *   lio_grid_convergence   get_grid_convergence (UP:119-122): atan(tan((lon - lon0) / 180 pi) sin(lat / 180 pi)) 180 / pi.
 *   lio_transform_from_rpyt   getTransformFromRPYT (SU:88-96): translation * Rz(yaw) * Rx(pitch) * Ry(roll), degrees through the truncated
 *               constant 0.01745329251994; row-major 4 x 4.
 *   lio_quat_of_transform     Eigen's Quaterniond(Matrix3d) of the rotation block, (w, x, y, z).
 *   lio_interpolate_transform interpolateTransform (SU:126-161) = the tail of RTKM::getInterpolatedTransform (RK:180-210): translation and
 *               angle-axis of pre^-1 next scaled by `ratio`, kEpsilon 1e-8.
 *   lio_rtk_transform_utm     computeRTKTransform(projector, data, zero_utm) (SU:112-124): UTM less zero_utm, altitude less zero_utm[2],
 *               yaw = -(heading - grid convergence at the projector's longitude0), getTransformFromRPYT(x, y, z, yaw, pitch, roll).
 *   lio_rtk_transform_origin  RTKM::computeRTKTransform(origin, data) (RK:125-139): the same with the origin fix projected again on every
 *               call and its altitude subtracted.
 *   lio_rtk_track   RTKM's mTimedInsData (RK:37-54, 91-95, 141-213): a map from stamp to fix (a fix with a stamp already held replaces it)
 *               with a projector of its own.  set_origin: the first one wins (1 = taken, 0 = one was set), T = the origin's own pose
 *               (mLastOdom).  feed: stored iff rtk_valid and the origin is set (1 / 0).  interpolate = getInterpolatedTransform, its
 *               refusals in the reference's order: no origin; [an exact stamp answers here: LIO_RTK_EXACT]; fewer than two fixes; stamp before
 *               the first; stamp after the last.  Otherwise the pair around the stamp with ratio = (t - pre) / (next - pre) (no + 1 here)
 *               through lio_interpolate_transform.  T is written only when the track answers.
 *   lio_gnss_queue  the graph's gps_queue (HG:141-156, 349-460, 653-660) up to the point where an edge is added.  set_origin: zero_utm =
 *               (easting, northing, altitude [- z of the last key frame's estimate when there is one]); every call replaces it.  push =
 *               gps_callback.  flush = flush_gps_queue over the key frames' stamps and has-fix flags (keyframe->utm_coord is set), in the
 *               reference's order: nothing without key frames or fixes; the cursor walk (a key frame later than the last fix ends it, one
 *               before the cursor's fix or with a fix is passed over); the bracket dt <= 0 && dt2 >= 0 && dt2 - dt < 2.0 (none found ends
 *               the walk); unequal precisions pass the key frame over; ratio = (t - pre) / (next - pre + 1) (HG:654-655); both fixes through
 *               lio_rtk_transform_utm and lio_interpolate_transform; z = 0 for dimension 2; the 10 / 20 / 50 m gate (precision < 100, < 1000,
 *               else) against last_xyz, the last accepted fix (gps_last_update_pose: the caller's, read and written; all zero = none yet);
 *               an accepted match sets the key frame's flag and last_xyz and is written to `out`; at the end every fix with a stamp <= the
 *               last key frame's is erased (upper_bound).  The quaternion is Quaterniond(rotation).normalize() as (x, y, z, w).  The
 *               reference flushes against `keyframes`, not `new_keyframes`: a key frame added in this pass is handed in at the next one.
 *               Returns the matches, or -(matches) when cap is too small -- the queue and the flags have moved all the same: cap = n_kf
 *               always suffices.  LIO_E_STATE without an origin.
 * ------------------------------------------------------------------------------------------------------------- */
typedef struct lio_utm lio_utm;
typedef struct lio_rtk_track lio_rtk_track;
typedef struct lio_gnss_queue lio_gnss_queue;
typedef struct lio_rtk_fix {  /* the fields of RTKType (slam/common/mapping_types.h:86-135) the GNSS side reads */
    uint64_t stamp_us;
    double latitude, longitude, altitude; /* degrees, degrees, metres */
    double heading, pitch, roll;          /* degrees */
    double precision;                     /* RTKType::precision (default 100) */
    int32_t dimension;                    /* RTKType::dimension: 2, 3 or 6 (default 2) */
    int32_t reserved;
} lio_rtk_fix;
typedef struct lio_gnss_match {
    int32_t keyframe;  /* index into the arrays handed to flush */
    int32_t dimension;
    uint64_t first_stamp_us, second_stamp_us; /* the pair of fixes around the key frame */
    double xyz[3];
    double quat[4];    /* x, y, z, w */
    double precision;
} lio_gnss_match;
#define LIO_RTK_INTERPOLATED 0
#define LIO_RTK_EXACT 1
#define LIO_RTK_NO_ORIGIN 2
#define LIO_RTK_TOO_FEW 3
#define LIO_RTK_EARLY 4
#define LIO_RTK_LATE 5
lio_utm* lio_utm_create(int zone_width);
void lio_utm_destroy(lio_utm*);
int lio_utm_zone(const lio_utm*);
int lio_utm_forward(lio_utm*, double latitude, double longitude, double* x, double* y);
int lio_utm_inverse(lio_utm*, double x, double y, double* latitude, double* longitude);
double lio_utm_longitude0(const lio_utm*);
double lio_grid_convergence(double longitude0, double lat, double lon);
void lio_transform_from_rpyt(double x, double y, double z, double yaw, double pitch, double roll, double T[16]);
void lio_quat_of_transform(const double T[16], double wxyz[4]);
void lio_interpolate_transform(const double pre[16], const double next[16], double ratio, double out[16]);
int lio_rtk_transform_utm(lio_utm*, const lio_rtk_fix* fix, const double zero_utm[3], double T[16]);
int lio_rtk_transform_origin(lio_utm*, const lio_rtk_fix* origin, const lio_rtk_fix* fix, double T[16]);
lio_rtk_track* lio_rtk_track_create(void);
void lio_rtk_track_destroy(lio_rtk_track*);
int lio_rtk_track_set_origin(lio_rtk_track*, const lio_rtk_fix* rtk, double T[16]);
int lio_rtk_track_origin(const lio_rtk_track*, lio_rtk_fix* out);
int lio_rtk_track_feed(lio_rtk_track*, int rtk_valid, const lio_rtk_fix* fix);
int lio_rtk_track_size(const lio_rtk_track*);
int lio_rtk_track_interpolate(const lio_rtk_track*, uint64_t stamp_us, double T[16]);
lio_gnss_queue* lio_gnss_queue_create(void);
void lio_gnss_queue_destroy(lio_gnss_queue*);
int lio_gnss_queue_set_origin(lio_gnss_queue*, const lio_rtk_fix* rtk, int have_keyframe, double last_keyframe_z, double zero_utm[3]);
int lio_gnss_queue_push(lio_gnss_queue*, const lio_rtk_fix* fix);
int lio_gnss_queue_size(const lio_gnss_queue*);
/* the stamps of the fixes held, in order: the count, or -(count) when cap is too small */
int lio_gnss_queue_stamps(const lio_gnss_queue*, uint64_t* stamps, uint32_t cap);
int lio_gnss_queue_flush(lio_gnss_queue*, const uint64_t* kf_stamps, uint8_t* kf_has_fix, uint32_t n_kf, double last_xyz[3], lio_gnss_match* out,
                         uint32_t cap);
/* graph_update_origin's coordinate change (HG:1396-1449), in place: a map recorded under the origin `from` expressed under the origin `to`.  Two
 * projectors made fresh as the reference makes them, each fixed to its zone by projecting its own origin (zero_utm_from, zero_utm_to).  Per
 * translation -- of each of the n_poses row-major 4 x 4 poses and of each of the n_xyz points (a GNSS prior's measurement): (lat, lon) =
 * inverse_from(x + zero_utm_from.x, y + zero_utm_from.y); (x, y) = forward_to(lat, lon) - zero_utm_to; z = z + from.altitude - to.altitude.
 * Rotations are not touched (the reference does not turn them by the difference in grid convergence).  Only latitude, longitude and altitude
 * of the two fixes are read.  Either array may be NULL with its count 0. */
int lio_update_origin(const lio_rtk_fix* from, const lio_rtk_fix* to, double* poses16, uint32_t n_poses, double* xyz, uint32_t n_xyz);

/* ---------------------------------------------------------------------------------------------------------------
 * Several lidars into one frame on the device (csrc/scanmerge.hip): mergePoints (slam/common/slam_utils.cpp:249-273) followed by
 * preprocessPoints (slam/common/slam_base.h:83-85) as RTKM::feedPointData calls them (slam/mapping/rtkm/src/rtkm.cpp:105-109), in one pass.
 *   input    L clouds (1 <= L <= 16), cloud 0 the base; each n_l points (x, y, z, intensity) f32, a uint32 stamp per point (us since the
 *            cloud's header) and a uint64 header stamp (us); scan_period_us (<= 2^32 - 1); the static transform (row-major 4 x 4 f64).
 *   keep     the base's points all, ungated.  For every other cloud time_shift = double(header_l) - double(header_0); stamp =
 *            double(stamp_i) + time_shift; kept iff stamp >= 0 && stamp <= double(scan_period_us) (slam_utils.cpp:261-264); the kept point's
 *            stamp becomes uint32_t(stamp) (:265).  early = stamp < 0, late = stamp > scan_period: counted per cloud.
 *   order    the base, then the clouds in the order given (the caller hands them in std::map order of their names), each in input order:
 *            a stable compaction.
 *   frame    every output point through pcl::transformPointCloud with a Matrix4d: the Matrix4d rule of lio_cloud_append_* (f64, terms left
 *            to right, one cast to f32, no contraction), by the same device function.  Intensity passes through.  Non-finite points are
 *            neither dropped nor counted: mergePoints has no such test.
 *   not carried   the point attribute's `id` column (PointAttr::id): nothing downstream reads it.  The merged header stamp is the base's.
 * ------------------------------------------------------------------------------------------------------------- */
typedef struct lio_scan_merge lio_scan_merge;
lio_scan_merge* lio_scan_merge_create(int device, uint32_t max_clouds, uint64_t max_points);
void lio_scan_merge_destroy(lio_scan_merge*);
int lio_scan_merge_set_transform(lio_scan_merge*, const double T[16]);
/* uploads the clouds, merges them; kept / early / late: n_clouds entries each or NULL (the base: kept = n_0, 0, 0); n_out: points of the frame */
int lio_scan_merge_run_host(lio_scan_merge*, uint32_t n_clouds, const float* const* xyzi, const uint32_t* const* stamps, const uint32_t* n_points,
                            const uint64_t* header_us, uint64_t scan_period_us, uint32_t* kept, uint32_t* early, uint32_t* late, uint64_t* n_out);
/* the frame of the last run: n x 4 f32 and n stamps; returns n, or -n when cap (points) is too small */
int64_t lio_scan_merge_download(lio_scan_merge*, float* xyzi, uint32_t* stamps, uint64_t cap);
/* the same on the device (float4 per point), valid until the next run on this handle */
const void* lio_scan_merge_device(lio_scan_merge*, const uint32_t** d_stamps, uint64_t* n);
/* device time (HIP events) of the last run: the uploads, count + scan + write + the count's read-back */
int lio_scan_merge_last_times(lio_scan_merge*, double* upload_us, double* merge_us);

/* ---------------------------------------------------------------------------------------------------------------
 * Lidar-INS calibration (csrc/calib_host.cpp, csrc/calib.hip; ABI 24): the reference's calib_ins_* chain -- the pybind module
 * sensor_driver/calibration/calib_wrapper.cpp:41-115 over lidar_ins/src/aligner.cpp and lidar_ins/src/sensor.cpp.
 *   cost      every key scan moved into the odometry frame by M_s = matrix(T_o0_ot_s * T_o_l) (f32; x' = ((m00 x + m01 y) + m02 z) + m03,
 *             separately rounded: the project's statement of pcl::transformPoint, which cannot be pinned without PCL), one exact k-NN index
 *             over the combined cloud, every point's K = k + 1 nearest in it (the point itself included, aligner.cpp:47-51), and
 *             sum over points and neighbours of min(d2, cap) with the cap compared with the SQUARED distance (aligner.cpp:25-28).
 *             metric 0 = global: k = 3, cap 10.0; metric 1 = local: k = 1, cap 1.0 (aligner.h:19-23).
 *   sum       DEVIATION: the reference adds the terms in f32 per batch of 1000 points and then over batches (aligner.cpp:22-72); this library
 *             returns the f64 sum in a fixed order (per point ascending, then a fixed tree), bit-identical from run to run.
 *   optimiser DEVIATION: nlopt's GN_DIRECT_L and LN_BOBYQA are replaced by lio_dfo_direct_l and lio_dfo_nelder_mead (below), restated from
 *             the published algorithms; the calling protocol of Aligner::lidarOdomTransform (aligner.cpp:82-190) is kept.
 *   a 7-float transform is tx, ty, tz, qw, qx, qy, qz; a 16-float one a row-major 4 x 4.
 * ------------------------------------------------------------------------------------------------------------- */
/* Scan::Scan (sensor.cpp:48-65): keep[i] = 1 iff the i-th draw of std::uniform_real_distribution<float>(0, 1) over
 * std::default_random_engine(stamp_us) is < min(1, 6000 / (n + 1)); the number kept */
int lio_calib_subsample(uint64_t n, int64_t stamp_us, uint8_t* keep);
/* Transform (transform.h:23-65) in f32 */
void lio_se3f_exp(const float v[6], float T[7]);
void lio_se3f_log(const float T[7], float v[6]);
void lio_se3f_mul(const float a[7], const float b[7], float out[7]);
void lio_se3f_inverse(const float a[7], float out[7]);
void lio_se3f_matrix(const float T[7], float M[16]);
void lio_se3f_from_matrix(const float M[16], float T[7]);
/* Odom::getOdomTransform (sensor.cpp:14-44) over m entries (stamps in us, T m x 7): the search runs forward from start_idx only, the ratio is
 * not clamped.  LIO_E_STATE for m < 2 (the reference reads past its vector) */
int lio_calib_interpolate(const int64_t* stamps, const float* T, uint32_t m, int64_t stamp, uint32_t start_idx, float T_out[7], uint32_t* match_idx);

/* derivative-free minimisers over a box (1 <= n <= LIO_DFO_MAX_DIM).  The hook runs after every evaluation; a non-zero return stops the
 * method.  Neither evaluates outside [lb, ub] or more than max_evals times.  x_best / report: the best point evaluated. */
#define LIO_DFO_MAX_DIM 8
#define LIO_DFO_STOP_EVALS 0
#define LIO_DFO_STOP_XTOL 1
#define LIO_DFO_STOP_HOOK 2
typedef double (*lio_dfo_fn)(const double* x, int n, void* user);
typedef int (*lio_dfo_hook)(int evals, const double* x, int n, double f, void* user);
typedef struct lio_dfo_params {
    int32_t max_evals; /* 500 */
    int32_t reserved;
    double xtol_abs;   /* 1e-4: DIRECT-L stops dividing a rectangle whose sides are all at most this, Nelder-Mead stops at such a simplex */
    double epsilon;    /* 1e-4: DIRECT-L's epsilon */
    double step[LIO_DFO_MAX_DIM]; /* Nelder-Mead: the initial simplex is x0 and x0 + step[i] e_i (- when + leaves the box); 0 = side / 20 */
} lio_dfo_params;
typedef struct lio_dfo_report {
    int32_t evals;
    int32_t stop;
    double f_best;
} lio_dfo_report;
void lio_dfo_default_params(lio_dfo_params*);
/* DIRECT (Jones, Perttunen & Stuckman 1993) with Gablonsky & Kelley's locally biased selection: first evaluation at the centre, no start point */
int lio_dfo_direct_l(lio_dfo_fn f, void* user, int n, const double* lb, const double* ub, const lio_dfo_params* p, lio_dfo_hook hook, void* hook_user,
                     double* x_best, lio_dfo_report* report);
/* Nelder-Mead (1965), coefficients 1, 2, 1/2, 1/2, every point projected onto the box */
int lio_dfo_nelder_mead(lio_dfo_fn f, void* user, int n, const double* x0, const double* lb, const double* ub, const lio_dfo_params* p,
                        lio_dfo_hook hook, void* hook_user, double* x_best, lio_dfo_report* report);

#define LIO_CALIB_MAX_SCANS 64
#define LIO_CALIB_GLOBAL 0
#define LIO_CALIB_LOCAL 1
#define LIO_CALIB_UNCAPPED 2 /* added to the metric: the walk starts from +inf instead of the cap (same terms; measurement only) */
typedef struct lio_calib_params { /* Aligner::Config (aligner.h:12-25) and the optimisers' own fields */
    int32_t local_only;       /* Config::local: skip the global stage */
    int32_t time_cal;         /* 1 */
    double max_time_offset;   /* 0.2 s */
    int32_t max_evals;        /* 500 per stage */
    int32_t knn_batch_size;   /* 1000: carried; the f64 sum has no batches */
    double xtol;              /* 1e-4 */
    int32_t local_knn_k;      /* 1 */
    int32_t global_knn_k;     /* 3 */
    float local_knn_max_dist; /* 1.0, compared with the squared distance */
    float global_knn_max_dist; /* 10.0 */
    double direct_epsilon;    /* 1e-4 */
    double nm_step[7];        /* Nelder-Mead's initial steps of the local stage: x, y, z (m), rotation vector (rad), time offset (s) */
} lio_calib_params;
typedef struct lio_calib_ins lio_calib_ins;
void lio_calib_default_params(lio_calib_params*);
/* NULL without a usable device */
lio_calib_ins* lio_calib_ins_create(int device);
void lio_calib_ins_destroy(lio_calib_ins*);
/* calib_ins_reset (calib_wrapper.cpp:41-54): no scans, no odometry, current = best = Transform(init) */
int lio_calib_ins_reset(lio_calib_ins*, const float init[16]);
/* Lidar::addPointcloud + Scan::Scan (sensor.cpp:102-114, 48-65): n points, `stride` floats apart (>= 3); every point is drawn for, a kept
 * point with a non-finite coordinate is dropped (the reference would trip FLANN's assertion); the points kept.  An empty scan is a scan.
 * LIO_E_CAPACITY beyond LIO_CALIB_MAX_SCANS (the limit of 20 is the wrapper's, calib_wrapper.cpp:61-65) */
int lio_calib_ins_add_scan(lio_calib_ins*, const float* xyz, uint64_t n, uint32_t stride, int64_t stamp_us);
/* Odom::addTransformData (sensor.cpp:10-12) */
int lio_calib_ins_add_odom(lio_calib_ins*, const float T[16], int64_t stamp_us);
int lio_calib_ins_counts(lio_calib_ins*, uint32_t* n_scans, uint32_t* n_odoms, uint64_t* n_points);
/* Lidar::setOdomLidarTransform(exp(x)) (aligner.cpp:97) */
int lio_calib_ins_set_transform(lio_calib_ins*, const double x[6]);
/* Lidar::setOdomOdomTransforms (sensor.cpp:122-127) at time_offset, then the S x 16 f32 matrices an evaluation at the current transform uses.
 * LIO_E_STATE with fewer than two odometry entries; LIO_E_INVALID when a pose is not finite (two entries with one stamp) */
int lio_calib_ins_scan_matrices(lio_calib_ins*, double time_offset, float* out);
/* Lidar::getCombinedPointcloud (sensor.cpp:116-120) at exp(x[0..6)), with nx == 7 at the time offset x[6] (nx == 6: the scan poses as they
 * were last set): n x 3 f32 in scan-major input order; the number of points */
int64_t lio_calib_ins_combined(lio_calib_ins*, const double* x, int nx, float* xyz_out, uint64_t cap);
/* Aligner::lidarOdomKNNError (aligner.cpp:33-80) as LidarOdomMinimizer calls it (:82-98), without the best-transform bookkeeping.
 * LIO_E_STATE with fewer than K points */
int lio_calib_ins_error(lio_calib_ins*, const double* x, int nx, int metric, double* err);
/* the n x K terms min(d2, cap) of that evaluation in combined-cloud index order, each row ascending: the test door */
int64_t lio_calib_ins_error_terms(lio_calib_ins*, const double* x, int nx, int metric, float* terms, uint64_t cap);
/* Aligner::lidarOdomTransform (aligner.cpp:137-190); blocks until done.  params NULL = the defaults */
int lio_calib_ins_calibrate(lio_calib_ins*, const lio_calib_params* params);
/* Aligner::getOptimizationStatus's inputs (aligner.cpp:192-199); may be called from another thread while _calibrate runs */
int lio_calib_ins_progress(lio_calib_ins*, int32_t* evals, double* best_err, int32_t* finished);
/* Lidar::getBestOdomLidarTransform().matrix() */
int lio_calib_ins_result(lio_calib_ins*, float T[16]);
/* device time (HIP events) of the last evaluation */
int lio_calib_ins_last_times(lio_calib_ins*, double* assemble_us, double* build_us, double* terms_us);

/* -------------------------------------------------------------------------------------------------------------
 * Lidar ground calibration on the device (csrc/calib_ground.hip): crop_points / test_point_in_polygon of calibration/lidar_calibration/
 * filter.py and is_colinear / get_plane_coefficient / fit_plane of fit.py, as calibration.py:calibrate_ground reaches them through
 * align_points_to_xyplane.  The rules are restated here; where the reference cannot be followed the rule is THE PROJECT'S and is marked so.
 * NULL from lio_calib_ground_create without a device: there is no CPU fallback.
 *   crop     everything in f64, the point's x and y widened from f32, the polygon's vertices f64 pairs.  Edge e runs from vertex p = e to
 *            q = e + 1, the last one back to vertex 0.  `up` is the vertex of the two with the strictly larger y, on equal y up = q; `down`
 *            is the other.  The edge counts iff down.y < y and y < up.y (both strict) and xi > x with
 *              xi = down.x + ((up.x - down.x) * (y - down.y)) / (up.y - down.y)            (in exactly this order, no fused multiply-add).
 *            A point is kept iff the number of counting edges is odd; a NaN x or y therefore drops the point, a NaN z does not.  The kept
 *            points keep their input order.  PROJECT: at most LIO_CALIB_GROUND_MAX_VERTICES vertices (the reference has no limit).
 *   planes   for a triple (i, j, k) into the cropped cloud, p1 = point i, p2 = point j, p3 = point k, all f32, every operation rounded to
 *            nearest on its own: u = p2 - p1, v = p3 - p1,
 *              a = u.y*v.z - v.y*u.z;  b = u.z*v.x - v.z*u.x;  c = u.x*v.y - v.x*u.y;
 *            colinear iff (|a| + |b|) + |c| < (float)1e-5;  norm = sqrtf((a*a + b*b) + c*c);  d = -((a*p1.x + b*p1.y) + c*p1.z);
 *            the plane is (a, b, c, d) / norm, all four negated when !(c > 0).  A colinear attempt has no plane (NaN in the log).
 *   score    the count of a plane is the number of cropped points with |((a*x + b*y) + c*z) + d| < (float)sigma in f32; a NaN distance
 *            does not count.  The device scores up to 128 attempts in one pass over the points.
 *   loop     fit_plane's, replayed on the host over the counts, attempts consumed in order: a colinear attempt is skipped and costs no
 *            iteration; an accepted attempt is one iteration: if (double)count > thresh * (double)n that plane wins and the loop ends (early
 *            exit), else a count strictly larger than the best so far (which starts at 0) makes it the best, the first of equal counts
 *            staying; the loop ends after num_iteration iterations.  Nothing found: every accepted count was 0, or every attempt colinear.
 *   draws    PROJECT (np.random.choice on numpy's global generator cannot be restated): attempt j is lio_ground_draw(seed, j, n), or, when
 *            the caller gives triples, triple j of that list; when the list is used up the loop ends with what it has.
 *            PROJECT: the loop gives up after 11 * num_iteration attempts (the reference loops forever over a cloud whose triples are all
 *            colinear).
 *   above    the ABI, in lsd_amd/calib_lidar.py (host, f64): the transform is the Rodrigues rotation of (a, b, c) onto (0, 0, 1) and the
 *            translation (0, 0, d / c), the quotient in f64 of the f32 coefficients.  PROJECT: parallel vectors give the identity (the
 *            reference divides 0 by 0 and returns NaN); ValueError names the reason for no plane found, fewer than 3 cropped points, fewer
 *            than 3 vertices and a winning plane with c == 0 (the reference fails by accident or answers with non-finite numbers).
 * ------------------------------------------------------------------------------------------------------------- */
#define LIO_CALIB_GROUND_MAX_VERTICES 256
typedef struct lio_calib_ground lio_calib_ground;
typedef struct lio_calib_ground_params {
    double sigma;          /* 0.05, compared as f32 */
    int32_t num_iteration; /* 100; 1 .. 10^6 */
    double thresh;         /* 0.9: the share of the cropped points that ends the loop early */
    uint32_t seed;         /* of the draws */
} lio_calib_ground_params;
/* the values align_points_to_xyplane passes (calib.py:25-27), seed 0 */
void lio_calib_ground_default_params(lio_calib_ground_params*);
lio_calib_ground* lio_calib_ground_create(int device);
void lio_calib_ground_destroy(lio_calib_ground*);
/* crop_points: n host points, stride_floats (>= 3) apart, x y z first, against the polygon of n_vertices (x, y) f64 pairs; the handle then
 * holds the kept points and *n_kept (may be NULL) their number, which may be 0.  LIO_E_INVALID for fewer than 3 or more than
 * LIO_CALIB_GROUND_MAX_VERTICES vertices or a stride below 3: nothing is touched, the previous crop stays downloadable */
int lio_calib_ground_crop_host(lio_calib_ground*, const float* xyz, uint64_t n, uint32_t stride_floats, const double* poly_xy, int n_vertices,
                               uint32_t* n_kept);
/* adopts a cloud as already cropped (fit_plane on its own): every point is held, position i is i */
int lio_calib_ground_set_points_host(lio_calib_ground*, const float* xyz, uint64_t n, uint32_t stride_floats);
/* fit_plane over the points the handle holds.  params NULL = the defaults.  triples NULL: the seeded draws; else n_triples x 3 indices into
 * the held points, consumed in order.  *found = 1 and coef = (a, b, c, d) of the winner, or *found = 0 and zeros (fit_plane's np.zeros(4)).
 * LIO_E_INVALID, the handle and the log of the last fit as they were: fewer than 3 points held, num_iteration outside 1 .. 10^6, a triple
 * with an index out of range or repeated */
int lio_calib_ground_fit(lio_calib_ground*, const lio_calib_ground_params* params, const uint32_t* triples, uint64_t n_triples, int* found,
                         float coef[4]);
/* each returns the number of items, or -(items) when cap is too small.  indices: the kept points' positions in the cropped cloud's input,
 * ascending; points: the held points, n x 3; draws: every attempt the device scored in the last fit (lio_calib_ground_last_run tells how many
 * the loop consumed): its triple, 1 if colinear, its count (0 if colinear) and its plane (NaN if colinear); any of the four may be NULL */
int64_t lio_calib_ground_download_indices(lio_calib_ground*, uint32_t* out, uint64_t cap);
int64_t lio_calib_ground_download_points(lio_calib_ground*, float* xyz, uint64_t cap);
int64_t lio_calib_ground_download_draws(lio_calib_ground*, uint32_t* triples, uint32_t* colinear, uint32_t* counts, float* planes, uint64_t cap);
/* the replay of the last fit: iterations (accepted attempts), attempts consumed, colinear attempts skipped, the winning attempt (-1: none) and
 * whether it won by the early exit */
int lio_calib_ground_last_run(lio_calib_ground*, int* iterations, int* attempts, int* skipped, int* winner, int* early_exit);
/* device time (HIP events on the handle's stream): the last crop's two kernels and scan; the last fit from its first launch to its last copy
 * (the host's replay between the batches included), and within it the plane and the score kernels summed over the batches */
int lio_calib_ground_last_times(lio_calib_ground*, double* crop_us, double* fit_us, double* planes_us, double* score_us);

/* ---------------------------------------------------------------------------------------------------------------
 * Lidar-IMU calibration: the IMU's mounting rotation from gyroscope samples and lidar rotations -- the reference's CalibLidarImu
 * (sensor_driver/calibration/lidar_imu/src/calib_lidar_imu.cpp) behind calib_imu_* (calib_wrapper.cpp:131-251).
 *
 * Host half (f64, no device; quaternions are (w, x, y, z); Eigen's rules restated, csrc/calib_imu_host.cpp):
 *   integrate    calib():291-301: rot[0] = I, rot[i] = rot[i-1] * (1, a/2), a = (g[i-1] + g[i]) / 2 * (t[i] - t[i-1]); neither the increment
 *                nor the product is normalised
 *   interpolate  getInterpolatedAttitude: scale == 0 or > 1 gives the identity; else q_s^-1 q_e normalised -> angle-axis -> the scaled angle
 *                through a rotation matrix back to a quaternion -> q_s * that, normalised
 *   time_align   calib():303-346: frames stamped before the first IMU sample are erased (*first_kept = how many); the walking IMU iterator
 *                (first sample not before the frame, one step back unless at the begin, kept across frames) gives the pair to interpolate
 *                between; the loop stops at the first frame whose second sample does not exist.  Frames first_kept .. first_kept +
 *                n_aligned - 1 get an attitude (quat_wxyz_out, n_frames x 4 is enough).  n_imu == 0: LIO_E_STATE
 *   solve        pairs: n x 8 (q_lidar, q_imu).  Each pair a 4 x 4 block huber * (L(q_imu) - R(q_lidar)), huber = 2 / angle_deg where
 *                angularDistance in degrees is above 2, else 1; the answer is the right singular vector of the smallest singular value of
 *                the 4n x 4 matrix (one-sided Jacobi on the matrix itself: the condition number is not squared).  Its sign is free: compare
 *                rotation matrices.  n == 0: the identity
 * The object:
 *   create       never touches the device: it is opened by the first call that handles a cloud (lio_calib_imu_lidar_pose, or add_frame with
 *                the flag set); LIO_E_DEVICE there when there is none (no CPU fallback).  max_scan_points bounds one frame, max_map_points
 *                the local map
 *   add_imu      n rows of 7 doubles (stamp us, gyro deg/s x 3, acc g x 3): / 1e6, / 180 * pi, * 9.81
 *   add_frame    addLidarData: (stamp / 1e6, global_T, delta_T) joins the frames; ignored (LIO_OK) from the 200th frame on.  With the "no RTK"
 *                flag set (lidar_pose was called) the rows are moved by global_T (f64, terms left to right, cast to f32: lio_cloud_append_*'s
 *                rule), filtered at 0.2 and appended to the map; the WHOLE map is filtered at 0.2 out of place into the target staging (the
 *                map itself is never replaced) and handed to lio_gicp_set_target_device.  Flag set and no map yet (the reference
 *                dereferences null): LIO_E_STATE.  More than max_scan_points rows, or a map past max_map_points: LIO_E_CAPACITY.  A point
 *                that is not finite: LIO_E_INVALID.  A refused call leaves the object as it was (the frame is not added either).  Without
 *                the flag (the RTK path) rows are not read and may be NULL
 *   lidar_pose   get_lidar_T_R: sets the flag.  n == 0: I and nothing else.  A kernel stages the strided rows (x y z intensity first,
 *                stride_floats >= 4) as float4 and counts the points whose x, y or z is not finite: any -> LIO_E_INVALID, nothing changed, the
 *                flag included.  The frame is filtered at 0.2 (lio_scan_voxel_downsample's semantics, intensity averaged).  First call: the map
 *                and the target are the RAW scan, the last pose and the answer are I.  Later: the filtered scan is the source
 *                (lio_gicp_set_source_device's rules: fewer than 20 points LIO_E_INVALID), the guess is the last pose rounded to f32,
 *                FAST_VGICP (voxel mode 1.0, DIRECT1, lio_estimate_matcher_params); not converged: I and the last pose stays; converged: the
 *                answer and the last pose are the result rounded to f32 (getFinalTransformation is a Matrix4f).  out_T row-major.
 *                No cloud crosses the link between the upload of the rows and out_T; the host reads back counts (the finite check, the
 *                filter's grid and voxel count) and the matcher's own round records
 *   calibrate    calib(true): integrate, time_align, pairs from delta_T's rotation of aligned frame i and the attitudes i-1, i, solve; R = the
 *                normalised result's matrix, row-major 3 x 3.  A second call without reset appends the aligned pairs again; erased frames
 *                stay erased.  No IMU sample, or no frame left: LIO_E_STATE (the reference reads past the end), R untouched
 *   lidar_poses / imu_poses  getLidarPose / getImuPose: the running products over the aligned frames from the second on, 16 doubles each;
 *                they return the number of poses, or -(poses) when cap is too small
 *   map_download / target_download  test visibility: the map in append order; the matcher's target in lio_gicp_download's internal order
 *   counts       frames held, IMU samples, aligned entries, map points, target points, the flag
 *   last_times   HIP events: staging, frame filter and matcher (set_source + align) of the last lidar_pose; the map update of the last add_frame
 *   set_max_iterations  a test hook: the matcher's iteration limit (64)
 * ------------------------------------------------------------------------------------------------------------- */
typedef struct lio_calib_imu lio_calib_imu;
int lio_calib_imu_integrate(const double* stamps_s, const double* gyr_rad, uint32_t n, double* quat_wxyz_out);
int lio_calib_imu_interpolate(const double q_s[4], const double q_e[4], double scale, double out[4]);
int lio_calib_imu_time_align(const double* imu_stamps_s, const double* imu_quat_wxyz, uint32_t n_imu, const double* frame_stamps_s, uint32_t n_frames,
                             uint32_t* first_kept, uint32_t* n_aligned, double* quat_wxyz_out);
int lio_calib_imu_solve(const double* pairs, uint32_t n, double quat_wxyz_out[4]);
lio_calib_imu* lio_calib_imu_create(int device, uint32_t max_scan_points, uint32_t max_map_points);
void lio_calib_imu_destroy(lio_calib_imu*);
int lio_calib_imu_reset(lio_calib_imu*);
int lio_calib_imu_add_imu(lio_calib_imu*, const double* rows7, uint32_t n);
int lio_calib_imu_add_frame(lio_calib_imu*, uint64_t stamp_us, const float* rows, uint32_t n, uint32_t stride_floats, const double global_T[16],
                            const double delta_T[16]);
int lio_calib_imu_lidar_pose(lio_calib_imu*, const float* rows, uint32_t n, uint32_t stride_floats, double out_T[16]);
int lio_calib_imu_calibrate(lio_calib_imu*, double R[9]);
int64_t lio_calib_imu_lidar_poses(lio_calib_imu*, double* out, uint64_t cap);
int64_t lio_calib_imu_imu_poses(lio_calib_imu*, double* out, uint64_t cap);
int64_t lio_calib_imu_map_download(lio_calib_imu*, float* xyzi, uint64_t cap);
int64_t lio_calib_imu_target_download(lio_calib_imu*, float* xyzi, uint64_t cap);
int lio_calib_imu_counts(lio_calib_imu*, uint32_t* frames, uint32_t* imus, uint32_t* aligned, uint32_t* map_points, uint32_t* target_points, int* no_rtk);
int lio_calib_imu_last_times(lio_calib_imu*, double* stage_us, double* filter_us, double* align_us, double* map_update_us);
int lio_calib_imu_set_max_iterations(lio_calib_imu*, int max_iterations);

/* ---------------------------------------------------------------------------------------------------------------
 * Detection boxes: the geometry around the reference's detection network -- the pybind11 module iou3d_nms_ext
 * (sensor_driver/inference/iou3d_nms/: iou3d_cpu.cpp, iou3d_nms_kernel.cu, iou3d_nms_api.cpp), sensor_driver/inference/iou3d_nms.py over it, and
 * the detector's post-process (sensor_inference/utils/model_nms_utils.py:4-22).  Boxes are rows of 7 f32: x y z dx dy dz heading.
 *
 *   pair      box_overlap, box_union and iou_bev of iou3d_cpu.cpp:118-312, statement for statement in f32 without contraction: corners rotated
 *             about the centre; the 16 edge-pair intersection tests in (i, j) order (check_rect_cross, the strict s1 * s2 > 0 && s3 * s4 > 0,
 *             the two formulas on either side of fabs(s5 - s1) > 1e-8); check_in_box2d with MARGIN 1e-2 and strict <, b's corners in a and a's
 *             in b interleaved per k; the centre is the f32 sum in insertion order over cnt; the points ascend by atan2f about it, equal keys
 *             in insertion order; the fan from point 0, fabs(area) / 2; cnt == 0 gives 0.  The hull: the eight corners under the bubble
 *             sort's exact passes with operator< (descending x then y, >=), the two monotone-chain passes with <= 0 pops and used[], the fan
 *             from hull point 0.  iou = overlap / fmaxf(dx_a dy_a + dx_b dy_b - overlap, 1e-8).  The device's cosf, sinf and atan2f are not
 *             glibc's: results differ from the reference's build by what last-bit differences of the three move (docs/kernels.md, "boxes")
 *   giou3d    boxes_giou3d_gpu of iou3d_nms.py:20-62 operation for operation in f32 (the tracker's matrix, sensor_fusion/MOT3D/model.py:44)
 *   nms       nms_gpu of iou3d_nms_api.cpp:49-85 with the sweep on the device: box i (in order) is kept when no kept box before it has
 *             iou_bev(kept, i) > thresh.  With scores the order is PROJECT's: descending score, ties to the smaller index, NaN last in index
 *             order -- np.argsort(-scores, kind="stable") (the reference's np.argsort(-scores) leaves ties to numpy's unstable default).
 *             LIO_BOXES_NMS_AABB_GATE ANDs in the gate of nms_cpu (iou3d_nms.py:78-129): the axis-aligned extents x -+ dx / 2, y -+ dy / 2,
 *             z -+ dz / 2 of the two boxes overlap strictly (min of the maxima > max of the minima) in all three
 *   post      class_agnostic_nms: box i passes when its label c (1-based) has an entry and score >= class_thresh[c - 1] (a negative entry
 *             means none; NaN never passes); the passing boxes in the order above through nms, the first post_max of the kept gathered.
 *             No host synchronisation between the upload and the one download (count and kept rows)
 * Errors: NULL from create without a device (no CPU fallback) or for max_boxes outside 1 .. 16384; LIO_E_INVALID for a NULL handle, a NULL
 * array with n > 0, more than max_boxes boxes on either side, an unknown mode.
 * ------------------------------------------------------------------------------------------------------------- */
#define LIO_BOXES_NMS_ROTATED 0
#define LIO_BOXES_NMS_AABB_GATE 1
typedef struct lio_boxes lio_boxes;
/* max_boxes: the most boxes on either side of any call */
lio_boxes* lio_boxes_create(int device, uint32_t max_boxes);
void lio_boxes_destroy(lio_boxes*);
/* host rows a (na x 7) and b (nb x 7); each output is row-major (na, nb) or NULL (not computed); na == 0 or nb == 0 writes nothing.
 * Replaces boxes_overlap_bev_gpu, boxes_union_bev_gpu, boxes_iou_bev_cpu (iou3d_nms_api.cpp:26-47, 87-143) and iou3d_nms.py:20-62 */
int lio_boxes_pairwise(lio_boxes*, const float* a, uint32_t na, const float* b, uint32_t nb, float* overlap, float* hull, float* iou_bev,
                       float* giou3d);
/* the number kept, their indices into the caller's arrays in keep (room for min(max_out, n)); scores NULL: the boxes are already in order;
 * max_out 0: no cap.  Replaces iou3d_nms_api.cpp:49-85 and the argsort / gather of iou3d_nms.py:64-76 (mode 0), iou3d_nms.py:78-129 (gate) */
int64_t lio_boxes_nms(lio_boxes*, const float* boxes, const float* scores, uint32_t n, float thresh, int mode, uint32_t max_out, int64_t* keep);
/* the mode of the two post-process entries below (NMS_TYPE nms_gpu = LIO_BOXES_NMS_ROTATED, the default; nms_cpu = LIO_BOXES_NMS_AABB_GATE) */
int lio_boxes_set_gate(lio_boxes*, int mode);
/* the number kept (at most post_max; 0 = no cap) and their rows, scores and labels in the outputs (room for min(post_max, n) each).
 * Replaces model_nms_utils.py:4-22 */
int64_t lio_boxes_postprocess(lio_boxes*, const float* boxes, const float* scores, const int32_t* labels, uint32_t n, const float* class_thresh,
                              int n_class, float nms_thresh, uint32_t post_max, float* out_boxes, float* out_scores, int32_t* out_labels);
/* the same with the three inputs in device memory (a network's heads never cross the link); the caller has finished writing them.  The
 * outputs are host arrays */
int64_t lio_boxes_postprocess_device(lio_boxes*, const float* d_boxes, const float* d_scores, const int32_t* d_labels, uint32_t n,
                                     const float* class_thresh, int n_class, float nms_thresh, uint32_t post_max, float* out_boxes,
                                     float* out_scores, int32_t* out_labels);
/* the positions in the caller's arrays of the boxes the last post-process kept, in its output order (from the same download: no device
 * traffic): their number, or -(number) when cap is too small; 0 after any other call */
int64_t lio_boxes_last_indices(lio_boxes*, uint32_t* out, uint64_t cap);
/* device time (HIP events) of the last nms or post-process: filter and order; prepare and mask; sweep; first launch to last.  After pairwise:
 * the total alone */
int lio_boxes_last_times(lio_boxes*, double* order_us, double* mask_us, double* sweep_us, double* total_us);

/* ---------------------------------------------------------------------------------------------------------------
 * Detection front end: what LidarInference::forward (sensor_driver/inference/tensorRT/lidar_inference.cpp:81-85) runs on every lidar frame
 * before the network -- the sliding window of sweeps (sensor_driver/inference/voxelize/preprocess_kernel.cu) and the hash voxeliser with its
 * mean VFE (voxelization_kernel.cu).  Rows are 5 f32: x y z intensity time.  The result is the reference's kernels run ONE THREAD AFTER
 * ANOTHER IN INDEX ORDER (one valid execution of the reference, and the only reproducible one), bit for bit.
 *
 *   grid      compute_grid_size (voxelization_kernel.cu:182-189): (int)std::round((max - min) / size) per axis in f32.  The product of the
 *             three must be below 2^32 - 1 (keys are 32 bits and 2^32 - 1 marks an empty slot)
 *   window    PreprocessImplement::forward (preprocess_kernel.cu:56-101) with num_feature 5: up to max_frame_num sweeps, newest first.  The
 *             caller's n is clamped to max_points (lidar_inference.cpp:81).  A realtime call drops the oldest sweep's count, clamps n to
 *             max(min(n, max_points - total), 1), shifts the counts, rewrites every remaining row behind the room of the new sweep
 *             (transform_kernel, :6-20): x y z = m[4r] * x + m[4r + 1] * y + m[4r + 2] * z + m[4r + 3] in f32, left to right, no contraction;
 *             channel 3 copied; channel 4 = (float)((double)t + 0.1); then the new sweep is copied to the front.  A non-realtime call empties
 *             the window and stores the sweep alone.  A call into a full window stores one row beyond max_points, as the reference does (its
 *             buffer has no room for it; the buffers here hold max_points + max_frame_num rows, the most that rule can reach)
 *   voxels    a point's coordinates are floorf((p - min) / size) per axis in IEEE f32; it counts when min <= p < max on all axes and the three
 *             indices are inside the grid (voxelization_kernel, :118-134).  Key (iz * gy + iy) * gx + ix.  A voxel's id is the rank of its
 *             first point in window order; voxels with id >= max_voxels and all their points vanish, num_voxels = min(real, max_voxels).  A
 *             voxel keeps its first max_points_per_voxel points in window order and its count is clamped to that
 *   features  reduce_mean_kernel (:158-180): per channel slot 0's value plus the others in slot order in f32, over (float)count, rounded to
 *             nearest-even f16 (subnormals kept, overflow to inf)
 *   indices   (0, z, y, x) for LIO_VOXEL_ORDER_ZYX (CenterPoint, the reference's call site), (0, x, y, z) for LIO_VOXEL_ORDER_XYZ
 * Deviations from the reference: a voxel exists only if a point passes BOTH tests (build_hash_table_kernel, :73-92, tests the
 * grid alone and creates voxels without points); points with a non-finite x, y or z are dropped before both passes (undefined there); a
 * non-realtime call zeroes the sweep counts (preprocess_kernel.cu:90 keeps stale ones).
 * Errors: NULL from create without a device (no CPU fallback) or on bad params (voxel size <= 0, max <= min, the grid's product too large,
 * max_points_per_voxel outside 1 .. 32, an unknown order, a zero max_voxels / max_points / max_frame_num); LIO_E_INVALID for a NULL handle
 * and for n == 0.
 * ------------------------------------------------------------------------------------------------------------- */
#define LIO_VOXEL_ORDER_XYZ 1
#define LIO_VOXEL_ORDER_ZYX 2
typedef struct lio_voxelizer_params {
    float min_range[3];
    float max_range[3];
    float voxel_size[3];
    uint32_t max_voxels;
    uint32_t max_points_per_voxel; /* 1 .. 32 */
    uint32_t max_points;           /* rows the window holds */
    uint32_t max_frame_num;        /* sweeps the window holds, >= 1 */
    int32_t order;                 /* LIO_VOXEL_ORDER_* */
} lio_voxelizer_params;
typedef struct lio_voxelizer lio_voxelizer;
/* host only: the grid of a range and a voxel size; LIO_E_INVALID for a size <= 0, max <= min or a non-finite value */
int lio_voxelize_grid_size(const float min_range[3], const float max_range[3], const float voxel_size[3], int out[3]);
lio_voxelizer* lio_voxelizer_create(int device, const lio_voxelizer_params*);
void lio_voxelizer_destroy(lio_voxelizer*);
/* forgets the window and the last result (inference_reset) */
int lio_voxelizer_reset(lio_voxelizer*);
/* one frame: host rows points (n x 5), the row-major 4 x 4 motion that takes the previous frame's coordinates to this frame's (read by
 * realtime calls only).  Returns the number of voxels.  One host wait.  Replaces lidar_inference.cpp:83-85 */
int64_t lio_voxelizer_forward(lio_voxelizer*, const float* points, uint32_t n, const float motion[16], int realtime);
/* the same with the rows in device memory (the caller has finished writing them): nothing is uploaded */
int64_t lio_voxelizer_forward_device(lio_voxelizer*, const float* d_points, uint32_t n, const float motion[16], int realtime);
/* the last result to host arrays with room for cap voxels: features (V x 5 f16 bit patterns), indices (V x 4), counts (V, clamped); each may
 * be NULL.  Returns V, or -V when cap is too small */
int64_t lio_voxelizer_output(lio_voxelizer*, uint16_t* features, int32_t* indices, uint32_t* counts, uint64_t cap);
/* the device addresses of the last result, valid until the next forward: what a sparse-convolution engine takes.  Returns V */
int64_t lio_voxelizer_output_device(lio_voxelizer*, const void** d_features, const int32_t** d_indices);
/* the window as it stands (rows x 5 f32, newest sweep first): the rows, or -(rows) when cap rows are too few */
int64_t lio_voxelizer_window(lio_voxelizer*, float* rows, uint64_t cap);
/* the rows of every sweep, newest first: max_frame_num, or -(max_frame_num) when cap is too small */
int64_t lio_voxelizer_window_counts(lio_voxelizer*, int32_t* per_frame, uint32_t cap);
/* the device address of the window's rows (rows x 5 f32), valid until the next forward or reset: the rows */
int64_t lio_voxelizer_window_device(lio_voxelizer*, const float** d_rows);
/* of the last forward: the voxels before the cap, the points that passed the tests, the points left in kept voxels' slots */
int lio_voxelizer_last_counts(lio_voxelizer*, uint64_t* real_voxels, uint64_t* points_in_range, uint64_t* points_kept);
/* device time (HIP events) of the last forward by stage: window move and sweep copy; table clear and insert; head ranking; slots; means; first
 * launch to last */
int lio_voxelizer_last_times(lio_voxelizer*, double* window_us, double* insert_us, double* rank_us, double* slots_us, double* mean_us,
                             double* total_us);

#ifdef __cplusplus
}
#endif
#endif /* LIO_HIP_H_ */
