/*
 * pcp_abi.h -- C ABI of libpcp: the MI355X-native hot path of
 * YamaguchiAtsushi/pointcloud_processor (crop/voxel -> SE(3)+concat -> virtual-LiDAR
 * ray-trace pose search), re-designed for gfx950.
 *
 * The reference has no plugin/operator/FFI API: its only stable interface is the ROS2
 * surface.  Each entry point below replaces one algorithm member function
 * of a reference node (cited file:line); a node shell keeps the topics/params/QoS and calls
 * these with the PointCloud2 buffers it already holds.  See INTEGRATION.md.
 *
 * Conventions
 *  - every function returns int status (PCP_OK = 0, < 0 on error) and never throws;
 *    the message is available from pcp_last_error(ctx).
 *  - a pcp_ctx owns one HIP device, one HIP stream and all device buffers.  It is NOT
 *    thread-safe (the reference runs callbacks on a single-threaded executor).
 *  - unless a `flags` argument says otherwise, pointers are HOST pointers owned by the
 *    caller; calls are synchronous (results are in host memory on return).
 *  - empty inputs are not errors: they return PCP_OK with zero outputs / best_idx = -1.
 *  - PCP_E_CAPACITY: an output buffer was too small; the *n_out argument holds the size
 *    that was needed and nothing else was written.
 */
#ifndef PCP_ABI_H
#define PCP_ABI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PCP_ABI_VERSION 2   /* 2: pcp_index_info.scan_layout */

enum pcp_status {
    PCP_OK = 0,
    PCP_E_INVALID = -1,   /* bad argument (null pointer, misaligned field, bad size) */
    PCP_E_HIP = -2,       /* HIP runtime / device error */
    PCP_E_CAPACITY = -3,  /* output capacity too small (*n_out = required) */
    PCP_E_STATE = -4,     /* missing prerequisite (e.g. pcp_set_cells not called) */
    PCP_E_NOMEM = -5      /* device or host allocation failed */
};

typedef struct pcp_ctx pcp_ctx;

/* A PointCloud2-like array-of-structs buffer: `n` points of `point_step` bytes each with
 * FLOAT32 x/y/z at byte offsets off_x/off_y/off_z (sensor_msgs::PointField).  Offsets and
 * point_step must be multiples of 4.  This is exactly what pcl::fromROSMsg reads. */
typedef struct pcp_cloud_view {
    const void *data;
    uint64_t n;
    uint32_t point_step;
    uint32_t off_x, off_y, off_z;
} pcp_cloud_view;

/* ---- context ----------------------------------------------------------------------- */
int pcp_abi_version(void);
int pcp_device_count(int *n);
int pcp_create(int device, pcp_ctx **out);
void pcp_destroy(pcp_ctx *ctx);
const char *pcp_last_error(const pcp_ctx *ctx);
int pcp_synchronize(pcp_ctx *ctx);

/* a second HIP stream of libpcp's own runtime on the context's device (e.g. the wait_stream of
 * pcp_raycast_fan_keys); the caller destroys it before the context */
int pcp_stream_create(pcp_ctx *ctx, void **stream);
int pcp_stream_destroy(pcp_ctx *ctx, void *stream);

/* device buffers owned by the caller (for inputs resident in HBM, e.g. benchmarks) */
int pcp_dev_alloc(pcp_ctx *ctx, uint64_t bytes, void **dptr);
int pcp_dev_free(pcp_ctx *ctx, void *dptr);
int pcp_memcpy_h2d(pcp_ctx *ctx, void *dst, const void *src, uint64_t bytes);
int pcp_memcpy_d2h(pcp_ctx *ctx, void *dst, const void *src, uint64_t bytes);
/* Pinned (page-locked) host memory for PointCloud2 data blobs: the node shell deserializes
 * into / publishes from these, so every H2D/D2H of the calls above runs as direct DMA instead
 * of the runtime's pageable staging.  pcp_host_register pins an existing buffer in place
 * (unregister before freeing it). */
int pcp_host_alloc(pcp_ctx *ctx, uint64_t bytes, void **hptr);
int pcp_host_free(pcp_ctx *ctx, void *hptr);
int pcp_host_register(pcp_ctx *ctx, void *hptr, uint64_t bytes);
int pcp_host_unregister(pcp_ctx *ctx, void *hptr);

/* process-wide counts of scratch (re)allocations by the library: device buffers, pinned
 * staging buffers, bytes allocated.  Each device reallocation frees the old buffer (a device
 * synchronization), so a streaming caller checks these settle after its first frames. */
int pcp_alloc_stats(uint64_t *device_reallocs, uint64_t *pinned_reallocs, uint64_t *bytes);

/* ---- in-library kernel timing (HIP events on the ctx stream) ------------------------ */
enum pcp_kernel_id {
    PCP_K_RAYCAST_FAN = 0,   /* fan ray-march (BASELINE configs[1], the headline)   */
    PCP_K_SCORE_CELLS,       /* mobile pose x cell ray-march + score                 */
    PCP_K_ZX120_CELLS,       /* pose-invariant zx120 cell evaluation                 */
    PCP_K_POSE_SUM,          /* ordered per-pose score sums                          */
    PCP_K_CELL_FLAGS,        /* stale-flag resolve + colour statistics              */
    PCP_K_CANDIDATES,        /* candidate lattice + ground height                    */
    PCP_K_INDEX_BUILD,       /* all kernels of a spatial index build                 */
    PCP_K_CROP,              /* crop-box stream compaction                           */
    PCP_K_VOXEL,             /* voxel keying + sort + centroid                       */
    PCP_K_TRANSFORM,         /* SE(3) + RGB + concat                                  */
    PCP_K_FILTER_MERGE,      /* whole crop->voxel->transform pipeline (graph replay)   */
    PCP_K_EXCAVATE,          /* excavated-terrain carve: heights + pit test + compaction */
    PCP_K_EXCAV_SETUP,       /* excavation-area normals + cell grid                    */
    PCP_K_VOXEL_REDO,        /* bucket-chain frames redone by the LSD chain (a bucket past
                              * its LDS capacity); launches = frames redone             */
    PCP_K_PLACE,             /* pcp_place_sensors' placement rounds (one launch per round)  */
    PCP_K_COUNT
};
int pcp_profile_enable(pcp_ctx *ctx, int enable);
int pcp_profile_reset(pcp_ctx *ctx);
int pcp_profile_get(pcp_ctx *ctx, int kernel_id, double *total_ms, uint64_t *launches);
const char *pcp_kernel_name(int kernel_id);

/* ---- pointcloud_filter (SimplifiedScanMatcher) --------------------------------------- */
/* cropFrontArea, pointcloud_filter.cpp:87-120 (predicate :111-113).  Order-preserving
 * strict box  box[0] < x < box[1], box[2] < y < box[3], box[4] < z < box[5]  with the
 * float coordinate compared to the double bound.  kept_idx (nullable): input indices of
 * the kept points, ascending.  out_xyz16 (nullable): kept points as PointXYZ (16-B
 * stride: x,y,z,1.0f). */
int pcp_crop_box(pcp_ctx *ctx, const pcp_cloud_view *in, const double box[6],
                 uint32_t *kept_idx, float *out_xyz16, uint64_t cap, uint64_t *n_kept);

/* downsampleCloud -> pcl::VoxelGrid<PointXYZ>, pointcloud_filter.cpp:122-139.
 * out_xyz16: centroids (PointXYZ, 16-B stride) in ascending voxel index.
 * voxel_idx / voxel_count (nullable): PCL's linear voxel index and points per voxel.
 * *passthrough = 1 when PCL's int32 index-overflow guard fires (output = input). */
int pcp_voxel_grid(pcp_ctx *ctx, const pcp_cloud_view *in, float leaf, float *out_xyz16,
                   uint32_t *voxel_idx, uint32_t *voxel_count, uint64_t cap, uint64_t *n_out,
                   int32_t *passthrough);

/* processCloudSimple, pointcloud_filter.cpp:64-85: crop then voxel (leaf <= 0: crop only)
 * fused on the device.  Output PointXYZ 16-B stride (the toROSMsg layout). */
int pcp_crop_voxel(pcp_ctx *ctx, const pcp_cloud_view *in, const double box[6], float leaf,
                   float *out_xyz16, uint64_t cap, uint64_t *n_out, uint64_t *n_cropped);

/* ---- pointcloud_merger (GnssGicpMatcher cloud part) ------------------------------------ */
typedef struct pcp_rigid {
    double t[3];   /* geometry_msgs Transform.translation */
    double q[4];   /* rotation x, y, z, w */
} pcp_rigid;

/* processPointClouds + processRobotCloud, pointcloud_merger.cpp:308-394: for each cloud i
 * in order, tf2::doTransform (float32 Eigen Translation3f*Quaternionf, :370) and tag colour
 * rgb[3i..3i+2] (:376-387), concatenated (robot first, then zx120, :316-325).
 * out_xyzrgb32: PointXYZRGB memory image, 32-B stride (x,y,z,1.0f,rgba,pad). */
int pcp_transform_concat(pcp_ctx *ctx, int k, const pcp_cloud_view *clouds,
                         const pcp_rigid *tf, const uint8_t *rgb, void *out_xyzrgb32,
                         uint64_t cap, uint64_t *n_out);

/* Full device pipeline (BASELINE configs[2]): per cloud crop -> voxel(leaf) -> transform +
 * colour, concatenated.  boxes: 6 doubles per cloud.  flags: PCP_MEM_DEVICE_IN (cloud data
 * pointers are device pointers) / PCP_MEM_DEVICE_OUT (out is a device pointer).
 * n_per_cloud (nullable, k entries): points each cloud contributed. */
#define PCP_MEM_DEVICE_IN 1u
#define PCP_MEM_DEVICE_OUT 2u
int pcp_filter_merge(pcp_ctx *ctx, int k, const pcp_cloud_view *clouds, const double *boxes,
                     float leaf, const pcp_rigid *tf, const uint8_t *rgb, void *out_xyzrgb32,
                     uint64_t cap, uint64_t *n_out, uint64_t *n_per_cloud, uint32_t flags);
/* The launch file's filter node (both sensors) and merger node composed in one process (a
 * component container; the C5 chain): per cloud i crop -> voxel(leaf), its centroids in its own
 * frame into filtered[i] (host, clouds[i].n PointXYZ 16-B records at most: the node's
 * /filtered_points message) AND all clouds transformed + coloured + concatenated into `out`
 * (host, PointXYZRGB 32-B, cap records: pcp_filter_merge's output), ONE synchronisation.  Host
 * memory in and out (message-sized clouds are read in place from pinned staging).  `out` and
 * each filtered[i] may be NULL (not copied: read them with pcp_filter_merge_landed).
 * n_per_cloud / n_cropped (nullable, k entries): centroids and cropped points of each cloud. */
int pcp_filter_merge_nodes(pcp_ctx *ctx, int k, const pcp_cloud_view *clouds,
                           const double *boxes, float leaf, const pcp_rigid *tf,
                           const uint8_t *rgb, void *out, uint64_t cap, uint64_t *n_out,
                           uint64_t *n_per_cloud, float *const *filtered, uint64_t *n_cropped);
/* Where the last pcp_filter_merge_nodes call's outputs landed: the context's pinned memory,
 * host-readable (the same bytes `out` / `filtered[i]` receive; a caller that reads them here may
 * pass out = NULL, filtered[i] = NULL to that call) -- merged: *n_out PointXYZRGB records,
 * filtered[i]: n_per_cloud[i] PointXYZ records.  A view over `merged` given to
 * pcp_excavate_area_async is read in place by the device (no staging copy).  Valid until the
 * context's next pcp_filter_merge*, pcp_transform_concat or pcp_excavate call; PCP_E_STATE when
 * there is none, or k differs from that call's. */
int pcp_filter_merge_landed(pcp_ctx *ctx, int k, const void **merged, const float **filtered);

/* ---- virtual_lidar (SimplifiedDualLidarOptimizer) -------------------------------------- */
typedef struct pcp_vl_params {      /* virtual_lidar.cpp:66-71 */
    double grid_resolution;         /* 0.1  */
    double sensor_height;           /* 1.1  */
    double search_radius;           /* 3.0  */
    double max_distance;            /* 15.0 */
    int32_t num_candidates;         /* 100  */
    int32_t vertical_layers;        /* 10   */
} pcp_vl_params;

/* GridCell flag bits (virtual_lidar.cpp:20-44) as kept by the caller between ticks */
#define PCP_F_RANGE_Z 1u
#define PCP_F_FOV_Z 2u
#define PCP_F_VIS_Z 4u
#define PCP_F_RANGE_M 8u
#define PCP_F_FOV_M 16u
#define PCP_F_VIS_M 32u

typedef struct pcp_vl_report {
    int64_t best_idx;            /* -1: no candidates */
    double best_score;           /* -inf when no candidates (:464) */
    double zx120_total_score;    /* evaluateZX120Only (:360-452) */
    int32_t zx120_range_ok, zx120_fov_ok, zx120_visible_ok;
    int32_t total_cells;
    int32_t zx120_green, zx120_red, zx120_blue, zx120_yellow;
    int32_t green, red, blue, yellow;   /* dual configuration (:480-519) */
} pcp_vl_report;

/* terrainCallback (:180-192): replaces KdTreeFLANN::setInputCloud(terrain).  n == 0 keeps
 * the previous index for ray casts (the reference keeps the stale tree) while ground
 * heights see the empty cloud (:601). */
int pcp_set_terrain(pcp_ctx *ctx, const pcp_cloud_view *terrain);
/* zx120PointsCallback (:194-207): index of /zx120/filtered_points for the relaxed check. */
int pcp_set_aux_cloud(pcp_ctx *ctx, const pcp_cloud_view *aux);
/* the valid cells of generateExcavationGrid3D (:236-287): centres (x,y,z double) and
 * surface normals (float, computeCellSurfaceNormal :301-340), in grid order. */
int pcp_set_cells(pcp_ctx *ctx, const double *xyz, const float *normals, uint64_t n);

/* excavationAreaCallback (virtual_lidar.cpp:164-178) on the GPU: replaces the excavation
 * KdTreeFLANN, computeTerrainNormals (:209-234: pcl::NormalEstimation, radius 1.5, viewpoint
 * (0,0,0), then flipped to normal_z >= 0) and generateExcavationGrid3D (:236-287, with
 * isPointNearExcavation :289-299 at radius 1.5 * grid_resolution and computeCellSurfaceNormal
 * :301-340).  The valid cells, in the reference's loop order, with their surface normals become
 * the context's scoring cells (as pcp_set_cells).  An empty area returns PCP_OK and keeps the
 * previous cells (:168).  grid_bbox (nullable out): grid_min_x, grid_max_x, grid_min_y,
 * grid_max_y, excavation_min_z, excavation_max_z after the margin; n_cells (nullable out).
 * `area` is host memory (the PointCloud2 data blob). */
int pcp_set_excavation_area(pcp_ctx *ctx, const pcp_cloud_view *area, double grid_resolution,
                            int32_t vertical_layers, double grid_bbox[6], uint64_t *n_cells);
/* The same setup, enqueued on the context's stream and NOT waited for (a composed chain: the
 * terrain and zx120 indices and the tick are enqueued behind it while it runs).  grid_bbox as
 * above (host arithmetic, exact at return); cells_cap: the lattice's points, an upper bound of
 * the cell count.  The count is settled -- and the neighbour lists regrown and rerun, should
 * they have overflowed -- by the next call that needs it: pcp_generate_and_score does so after
 * its own synchronisation (ONE wait for both; its cell_flags must then hold cells_cap bytes,
 * are taken as fresh GridCells -- all clear, :259 -- and come back for the settled count), every
 * other call that reads the cells (pcp_score_poses, pcp_get_cells, pcp_set_cells, the multi
 * calls, another setup) before it starts.  Results are identical to pcp_set_excavation_area's. */
int pcp_set_excavation_area_async(pcp_ctx *ctx, const pcp_cloud_view *area,
                                  double grid_resolution, int32_t vertical_layers,
                                  double grid_bbox[6], uint64_t *cells_cap);
/* the context's scoring cells (settles a pending setup: may wait for the stream) */
int pcp_cells_count(pcp_ctx *ctx, uint64_t *n_cells);
/* ---- excavated_surface_generator.cpp (ExcavationTerrainGenerator) ------------------------ */
typedef struct pcp_excavation_params {   /* excavated_surface_generator.cpp:29-51 */
    double depth;                 /* excavation.depth 1.0 */
    double slope_angle_deg;       /* excavation.slope_angle 75.0 */
    double offset_x, offset_y;    /* excavation.offset_x/_y 4.0, 1.0 (zx120 base frame) */
    double point_density;         /* excavation.point_density 0.05 */
    double terrain_search_radius; /* excavation.terrain_search_radius 0.5 */
    int32_t l_shape_enabled;      /* excavation.l_shape_enabled 1 */
    double arm1_length, arm1_width, arm2_length, arm2_width;   /* 2.0 1.2 2.0 1.2 */
    double width, length;         /* rectangle mode 1.2, 1.8 */
} pcp_excavation_params;

/* matchedCloudCallback (:259-326) with excavation enabled and the zx120 TF present
 * (zx120_base = map -> zx120/base_link).  in: /matched_point_cloud, host memory (x/y/z float
 * fields; the rgb float at byte 16 when point_step >= 20, else 0).  Outputs are PointXYZRGB
 * records (32 B: x, y, z, 1, rgb, 0, 0, 0) in host buffers:
 *   terrain_out: /excavated_terrain = the input points processExcavation keeps (:451-485,
 *                input order) then generateExcavatedSurface's bottom and wall points (:487-584)
 *   area_out:    /excavation_area = generateExcavationArea (:350-455)
 * Every getTerrainHeight (:183-226) runs on the GPU against one index of the input (the
 * reference rebuilds a KD-tree per call, once per input point).  A height that is a mean is
 * the exactly rounded sum of its m neighbours' z over m (to one ulp: the double-double's final
 * rounding); it is the reference's bits whenever the reference's own sequential double sum is
 * exact -- sufficient: every z within the radius a multiple of one quantum u with
 * m * max|z| < 2^53 * u (e.g. u = 2^-42: every such float z zero or |z| >= 2^-19, which the
 * default radius keeps below 0.5, and m <= 1024).  Past that the reference's sum depends on its
 * neighbour order and the two can differ in the mean's last bits.  pose_out (nullable): the
 * excavation centre x, y, its terrain height, yaw (publishExcavationMarkers).  *_cap in
 * records; PCP_E_CAPACITY with *n_* set when short.  A missing TF is the caller's branch
 * (:276-279: the input is republished unchanged). */
int pcp_excavate(pcp_ctx *ctx, const pcp_cloud_view *in, const pcp_excavation_params *p,
                 const pcp_rigid *zx120_base, void *terrain_out, uint64_t terrain_cap,
                 uint64_t *n_terrain, void *area_out, uint64_t area_cap, uint64_t *n_area,
                 double pose_out[4]);
/* The carve node and virtual_lidar's two callbacks for its messages composed in one process
 * (the C5 chain): pcp_excavate, then pcp_set_excavation_area_async over /excavation_area
 * (skipped when empty: :168) and pcp_set_terrain over /excavated_terrain, fed from the carve's
 * records where they land (device-readable pinned memory, no staging copy or upload), the host
 * copies into terrain_out / area_out made after the setup and the index build are enqueued.
 * Arguments and results as those three calls'; grid_bbox / cells_cap as
 * pcp_set_excavation_area_async's (settled the same way).  Waits once (the carve's counts).
 * terrain_out = area_out = NULL: nothing is copied (the caps are not checked); the records stay
 * where they landed, read with pcp_excavate_landed -- a composed caller enqueues its next
 * consumers (the zx120 index) first and builds its messages from there. */
int pcp_excavate_area_async(pcp_ctx *ctx, const pcp_cloud_view *in,
                            const pcp_excavation_params *p, const pcp_rigid *zx120_base,
                            void *terrain_out, uint64_t terrain_cap, uint64_t *n_terrain,
                            void *area_out, uint64_t area_cap, uint64_t *n_area,
                            double pose_out[4], double grid_resolution, int32_t vertical_layers,
                            double grid_bbox[6], uint64_t *cells_cap);
/* Where the last pcp_excavate_area_async call made with null outputs left its records: the
 * context's pinned memory, host-readable -- terrain: *n_terrain, area: *n_area PointXYZRGB
 * records of that call (the bytes terrain_out / area_out would have received).  Valid until the
 * context's next pcp_excavate* call; PCP_E_STATE when there is none. */
int pcp_excavate_landed(pcp_ctx *ctx, const void **terrain, const void **area);

/* ---- calc_drivable_area.cpp (the occupancy-grid node) -------------------------------------- */
typedef struct pcp_drivable_params {   /* calc_drivable_area.cpp:20-26 */
    double grid_resolution;            /* 1.0 */
    double map_width, map_height;      /* 100, 100 */
    double max_gradient;               /* 0.3 */
    int32_t min_points_per_cell;       /* 10 */
    double start_clear_radius;         /* 3.0 */
} pcp_drivable_params;

/* robotCloudCallback (:67-226): the robot's filtered cloud (host memory, sensor frame) through
 * tf2::doTransform(cloud_to_map) (Eigen float), binned into the grid centred on (robot_x,
 * robot_y) (map -> four_wheel_robot/base_link); start_x/y = the first robot position (the
 * node's state).  grid (dims[1] rows of dims[0] int8, row-major over y): 0 free, 100 obstacle,
 * -1 unknown -- nav_msgs/OccupancyGrid.data; origin = the grid's lower-left corner.  An empty
 * cloud publishes nothing (:107-111): PCP_OK, grid untouched. */
int pcp_drivable_area(pcp_ctx *ctx, const pcp_cloud_view *cloud, const pcp_rigid *cloud_to_map,
                      double robot_x, double robot_y, double start_x, double start_y,
                      const pcp_drivable_params *p, int8_t *grid, uint64_t cap, int32_t dims[2],
                      double origin[2]);

/* upper bounds of pcp_excavate's record counts for an n-point input (host arithmetic only) */
int pcp_excavate_bounds(const pcp_excavation_params *p, uint64_t n_in, uint64_t *terrain_cap,
                        uint64_t *area_cap);

/* the context's scoring cells: xyz (n x 3 double) and normals (n x 3 float), either nullable;
 * *n_cells = count (PCP_E_CAPACITY when it exceeds cap). */
int pcp_get_cells(pcp_ctx *ctx, double *xyz, float *normals, uint64_t cap, uint64_t *n_cells);
/* terrain_normals_ of the last pcp_set_excavation_area, in input order (n x 3 float, NaN
 * where fewer than 3 neighbours or a non-finite point). */
int pcp_get_area_normals(pcp_ctx *ctx, float *normals, uint64_t cap, uint64_t *n);

/* generateCandidatePositions + getGroundHeight (:550-625).  grid_bbox = {grid_min_x,
 * grid_max_x, grid_min_y, grid_max_y, excavation_min_z, excavation_max_z} after the
 * margin (:251-254).  zx120_pose5 = {x,y,z,pitch,yaw} from getZX120Position (:342-358).
 * poses5 out: x,y,z,pitch,yaw per candidate, in the reference's lattice order. */
int pcp_generate_candidates(pcp_ctx *ctx, const double grid_bbox[6], const pcp_vl_params *p,
                            const double zx120_pose5[5], double *poses5, uint64_t cap,
                            uint64_t *n_out);

/* runOptimization's scoring (:460-519): evaluateZX120Only, evaluatePosition per candidate
 * (:627-654), strict-'>' argmax (:471-474) and the colour statistics from the stale
 * GridCell flags (:487-501).  cell_flags: in/out, one byte per cell (PCP_F_*), the state
 * the caller's GridCells hold.  total_score/covered (nullable): per candidate. */
int pcp_score_poses(pcp_ctx *ctx, const double *poses5, uint64_t n, const double zx120_pose5[5],
                    const pcp_vl_params *p, uint8_t *cell_flags, double *total_score,
                    int32_t *covered, pcp_vl_report *rep);

/* Diagnostics of the reference's own ray march (the roofline of k_score_cells, bench.py
 * reference_mode; never used for results).  pcp_score_poses_stats: the query's visibility rays
 * (the same rows, cells and march as pcp_score_poses) counted by a twin of the kernel --
 * stats[0] z-band probes (2-byte records), stats[1] candidates' walk starts (4 bytes),
 * stats[2] point records tested (12 bytes), stats[3] directory loads (0 with the fine-window
 * copy).  pcp_score_poses_burst: the query's production k_score_cells launch `reps` times
 * back-to-back between two stream events; *ms_per_launch = the interval / reps.  Neither
 * touches the caller's GridCell flags. */
/* evaluateCellScore's value for every (pose, cell) of the query (k_score_cells' rows, before
 * evaluatePosition's std::max): score_mobile [n][n_cells], score_zx120 [n_cells] (host).  The
 * per-cell parity bar (tests); the caller's GridCell flags are not touched. */
int pcp_score_matrix(pcp_ctx *ctx, const double *poses5, uint64_t n, const double zx120_pose5[5],
                     const pcp_vl_params *p, double *score_mobile, double *score_zx120);
int pcp_score_poses_stats(pcp_ctx *ctx, const double *poses5, uint64_t n,
                          const double zx120_pose5[5], const pcp_vl_params *p, uint64_t stats[4]);
int pcp_score_poses_burst(pcp_ctx *ctx, const double *poses5, uint64_t n,
                          const double zx120_pose5[5], const pcp_vl_params *p, int reps,
                          double *ms_per_launch);

/* runOptimization's device part in one call (:455-519): pcp_generate_candidates then
 * pcp_score_poses on those candidates, identical results, one synchronisation -- the scoring
 * reads the candidates and their count where the generation left them on the device (the
 * reference's generateCandidatePositions + candidate loop).  poses5 (cap poses) receives the
 * candidates, *n_out their count; the rest as pcp_score_poses.  Lattices past 65,535 points
 * run as the two calls. */
int pcp_generate_and_score(pcp_ctx *ctx, const double grid_bbox[6], const pcp_vl_params *p,
                           const double zx120_pose5[5], double *poses5, uint64_t cap,
                           uint64_t *n_out, uint8_t *cell_flags, double *total_score,
                           int32_t *covered, pcp_vl_report *rep);

/* Greedy placement of several mobile sensors: runOptimization's "best of one" (:460-475)
 * generalised.  A cell's combined score is the max over zx120 and every placed sensor, a pose's
 * total the ordered sum of the positive combined scores (evaluatePosition, :627-654).  With
 * S[p][c], Z[c] the values pcp_score_matrix returns for the same arguments, max(a, b) the
 * reference's std::max ((a < b) ? b : a) and osum(v) the sum, in cell order from +0.0, of the
 * elements with v[c] > 0:  base = Z, T = osum(base) (*zx120_total, pcp_vl_report's
 * zx120_total_score), *zx120_covered = #{Z > 0}, owner[c] = Z[c] > 0 ? PCP_OWNER_ZX120 :
 * PCP_OWNER_NONE, every pose alive.  Round r = 0 .. k_max - 1: stop when no pose is alive;
 * t[p] = osum(max(base[c], S[p][c])) and cov[p] = #{.. > 0} for the alive poses (round_totals
 * [r][p]; -inf for the others); b = the first maximum (strict '>', :471-474); stop unless
 * t[b] > T (no pose adds anything); selected[r] = b, total_after[r] = T = t[b], covered_after[r]
 * = cov[b]; every cell with base[c] < S[b][c] gets owner r and base[c] = S[b][c] (ties keep the
 * earlier owner); b leaves the search, and with min_separation > 0 so does every pose p with
 * dx * dx + dy * dy < min_separation * min_separation (dx = x_p - x_b, dy = y_p - y_b, double,
 * each operation rounded).  *n_selected = rounds recorded; entries and rows from there on are not
 * written; cell_score = base.  One synchronisation; the caller's GridCell flags are neither read
 * nor written.  n <= 65535; PCP_E_INVALID (before any launch) for k_max outside 1 ..
 * PCP_PLACE_MAX, reserved != 0 or a step table past PCP_MAX_STEPS.  n == 0 or no cells: PCP_OK,
 * *n_selected = 0. */
#define PCP_PLACE_MAX 16
#define PCP_OWNER_ZX120 (-1)
#define PCP_OWNER_NONE  (-2)
typedef struct pcp_place_params {
    int32_t k_max;          /* sensors to place, 1 .. PCP_PLACE_MAX */
    int32_t reserved;       /* 0 */
    double min_separation;  /* metres in XY between placed poses; <= 0: no constraint */
} pcp_place_params;
int pcp_place_sensors(pcp_ctx *ctx, const double *poses5, uint64_t n,
                      const double zx120_pose5[5], const pcp_vl_params *p,
                      const pcp_place_params *pp,
                      int64_t *selected,        /* [k_max] pose index per round            */
                      double *total_after,      /* [k_max] total with sensors 0..r placed   */
                      int32_t *covered_after,   /* [k_max] covered cells, same             */
                      double *round_totals,     /* nullable [k_max][n]                      */
                      double *cell_score,       /* nullable [n_cells] final combined score  */
                      int32_t *cell_owner,      /* nullable [n_cells] round index / PCP_OWNER_* */
                      double *zx120_total, int32_t *zx120_covered, /* nullable */
                      int32_t *n_selected);

/* The exact best pair of mobile sensors: every pair of the poses evaluated, not greedy rounds (the
 * best pair need not contain the best single pose, which is where pcp_place_sensors starts).
 * S[p][c], Z[c], max(a, b) and osum(v) as above; fixed[0 .. n_fixed) are poses already placed.
 *   1. base = Z; for i = 0 .. n_fixed - 1 in list order base = max(base, S[fixed[i]]);
 *      owner[c] = Z[c] > 0 ? PCP_OWNER_ZX120 : PCP_OWNER_NONE, then fixed sensor i owns every
 *      cell where base[c] < S[fixed[i]][c] held at its fold (ties keep the earlier owner);
 *      *base_total = osum(base), *base_covered = #{base > 0} (n_fixed = 0: pcp_place_sensors'
 *      zx120_total / zx120_covered).
 *   2. Pose p is admissible iff it is not in fixed and, with min_separation > 0, for no fixed f
 *      dx * dx + dy * dy < min_separation * min_separation (pcp_place_sensors' expression, each
 *      operation rounded).
 *   3. s[p] = osum(max(base, S[p])) for admissible p, -inf otherwise (single_totals [n]);
 *      *best_single = the first maximum (strict '>' from -inf), -1 when no pose is admissible;
 *      *single_total / *single_covered its total and #{.. > 0} (-inf / 0 without one).
 *   4. For a < b, both admissible and (min_separation > 0) not closer to each other than it:
 *      t[a][b] = osum(max(max(base, S[a]), S[b])); pair_totals [n][n] holds t[a][b], every other
 *      entry -inf (the diagonal, the lower triangle, inadmissible pairs); best_pair = the first
 *      maximum in row-major order (a ascending, then b; strict '>'), (-1, -1) when there is no
 *      admissible pair; *pair_total / *pair_covered its values (-inf / 0 without one).
 *   5. *n_selected = 2 when a pair exists and *pair_total > *single_total; otherwise 1 when a
 *      single exists and *single_total > *base_total; otherwise 0 (under a separation the best
 *      pair can lose to the best single).  cell_score / cell_owner describe that answer: the
 *      base, then the chosen pose or poses folded in the order a, b with owners n_fixed and
 *      n_fixed + 1, ties to the earlier owner.
 * PCP_E_INVALID before any launch, nothing written: n_fixed outside 0 .. PCP_PLACE_MAX, reserved
 * != 0, a fixed index >= n or listed twice, n > PCP_PAIR_MAX_POSES, a step table past
 * PCP_MAX_STEPS, a null required pointer (everything not marked nullable), a null context.
 * n == 0 or no cells: PCP_OK, *n_selected = 0, *best_single = -1, best_pair = (-1, -1), the base
 * totals as defined (0 without cells).  One synchronisation; deterministic (two calls give
 * identical bytes); the caller's GridCell flags are neither read nor written; the call's scratch
 * is its own, so the other queries on the context are unchanged by it. */
#define PCP_PAIR_MAX_POSES 2048
typedef struct pcp_pair_params {
    int32_t n_fixed;                 /* sensors already placed, 0 .. PCP_PLACE_MAX */
    int32_t reserved;                /* 0 */
    double  min_separation;          /* metres in XY; <= 0: no constraint */
    int64_t fixed[PCP_PLACE_MAX];    /* indices into poses5, first n_fixed used */
} pcp_pair_params;
int pcp_place_pair(pcp_ctx *ctx, const double *poses5, uint64_t n, const double zx120_pose5[5],
                   const pcp_vl_params *p, const pcp_pair_params *pp,
                   int64_t best_pair[2], double *pair_total, int32_t *pair_covered,
                   int64_t *best_single, double *single_total, int32_t *single_covered,
                   double *base_total, int32_t *base_covered,
                   double *pair_totals,    /* nullable [n][n]  */
                   double *single_totals,  /* nullable [n]     */
                   double *cell_score, int32_t *cell_owner,   /* nullable [n_cells] */
                   int32_t *n_selected);

/* Kernel timing of pcp_place_pair (the timing tool only): the query's setup (the scoring) once,
 * then `reps` repetitions of its pair phase -- preparation, pair tiles, selection, no dense table
 * -- between two stream events; *ms_per_rep = the interval / reps.  n >= 1, cells present. */
int pcp_place_pair_burst(pcp_ctx *ctx, const double *poses5, uint64_t n, const double zx120_pose5[5],
                         const pcp_vl_params *p, const pcp_pair_params *pp, int reps, double *ms_per_rep);

/* The exact best triple of mobile sensors: every triple of the poses evaluated (greedy's three can
 * be 1-exchange optimal and still not the best three: two sensors may have to move together).
 * S[p][c], Z[c], max(a, b), osum(v), base, the owners, admissibility and the separation expression
 * are pcp_place_pair's, and so is pp.
 *   1.-4. pcp_place_pair's steps 1 to 4: *base_total / *base_covered, the singles with
 *      *best_single / *single_total / *single_covered, the pairs with best_pair / *pair_total /
 *      *pair_covered -- the values that call returns for the same arguments (its dense tables are
 *      not returned here).
 *   5. For a < b < c, all three admissible and (min_separation > 0) no two of them closer to each
 *      other than it: t[a][b][c] = osum(max(max(max(base, S[a]), S[b]), S[c])); triple_totals
 *      [n][n][n] holds t[a][b][c], every other entry -inf.  first_totals[a] = the first maximum
 *      of t[a][.][.] over (b, c) in row-major order (b ascending, then c; strict '>' from -inf),
 *      first_partners[a] its (b, c); -inf and (-1, -1) where pose a starts no triple.
 *      best_triple = the first maximum over a of first_totals, i.e. the lexicographically first
 *      maximal triple, (-1, -1, -1) when there is no admissible triple; *triple_total /
 *      *triple_covered its total and its count of positive elements (-inf / 0 without one).
 *   6. The answer: T = *base_total, *n_selected = 0; if a single exists and *single_total > T:
 *      *n_selected = 1, T = *single_total; if a pair exists and *pair_total > T: *n_selected = 2,
 *      T = *pair_total; if a triple exists and *triple_total > T: *n_selected = 3.  (A single's or
 *      a pair's total is never below the base's, so the first two steps are pcp_place_pair's
 *      rule; under a separation the best triple can lose to a pair or a single.)  cell_score /
 *      cell_owner describe that answer: the base, then the chosen poses folded in ascending index
 *      order with owners n_fixed, n_fixed + 1, n_fixed + 2, ties to the earlier owner.
 * PCP_E_INVALID before any launch, nothing written: everything pcp_place_pair refuses, n >
 * PCP_TRIPLE_MAX_POSES, triple_totals given with n > PCP_TRIPLE_TABLE_MAX_POSES, a null required
 * pointer (everything not marked nullable), a null context.  n == 0 or no cells: PCP_OK,
 * *n_selected = 0, every index -1, the base totals as defined (0 without cells); n < 3 just has no
 * triple.  One synchronisation; deterministic (two calls give identical bytes); the caller's
 * GridCell flags are neither read nor written; the call's scratch is its own, so the other queries
 * on the context are unchanged by it. */
#define PCP_TRIPLE_MAX_POSES        512   /* 22.2 M triples */
#define PCP_TRIPLE_TABLE_MAX_POSES  128   /* the dense table is offered up to here (16.8 MB) */
int pcp_place_triple(pcp_ctx *ctx, const double *poses5, uint64_t n, const double zx120_pose5[5],
                     const pcp_vl_params *p, const pcp_pair_params *pp,   /* the pair call's struct */
                     int64_t best_triple[3], double *triple_total, int32_t *triple_covered,
                     int64_t best_pair[2], double *pair_total, int32_t *pair_covered,
                     int64_t *best_single, double *single_total, int32_t *single_covered,
                     double *base_total, int32_t *base_covered,
                     double *first_totals,    /* nullable [n]       */
                     int64_t *first_partners, /* nullable [n][2]    */
                     double *triple_totals,   /* nullable [n][n][n] */
                     double *cell_score, int32_t *cell_owner,   /* nullable [n_cells] */
                     int32_t *n_selected);

/* Kernel timing of pcp_place_triple (the timing tool only): the query's setup (the scoring) once,
 * then `reps` repetitions of its triple phase -- the pair phase it builds on (preparation, pair
 * tiles, selection), the triple tiles, the rows' maxima and the selection, no dense table --
 * between two stream events; *ms_per_rep = the interval / reps.  n >= 3, cells present. */
int pcp_place_triple_burst(pcp_ctx *ctx, const double *poses5, uint64_t n, const double zx120_pose5[5],
                           const pcp_vl_params *p, const pcp_pair_params *pp, int reps,
                           double *ms_per_rep);

/* 1-exchange refinement of a placement: a set of k sensors (greedy's answer, or a deployment as
 * it stands) is improved by moving one sensor at a time to the pose that raises the total most,
 * until no single move raises it.  S[p][c], Z[c], max(a, b), osum(v) and the separation expression
 * as in pcp_place_sensors; fold(list) = Z with S[q] folded in, q in list order, by max.
 *   1. s = start; T = osum(fold(s)) is *start_total, *start_covered = #{fold(s) > 0}.
 *   2. One evaluation: for every slot i >= n_locked, L_i = fold(s without slot i) and
 *      u[i][p] = osum(max(L_i, S[p])) with its count of positive elements; u[i][p] = -inf where
 *      the move is inadmissible: slot i is locked (i < n_locked); p is in s (any slot, i included);
 *      or, with min_separation > 0, p is closer than it to some s_j, j != i.  Only the incoming
 *      pose is tested: the start set itself need not respect the separation, and a sensor that
 *      stays is never moved or refused for it.  swap_totals[e] holds evaluation e's whole [k][n]
 *      table.
 *   3. The best entry is the first maximum in row-major order (slot ascending, then pose; strict
 *      '>' from -inf).
 *   4. If it is not > T (or there is none): *converged = 1, stop.  If max_moves moves are recorded
 *      already: stop with *converged = 0.
 *   5. Otherwise move m = (move_slot = i, move_from = s_i, move_to = p, move_total = u[i][p],
 *      move_covered = its count); s_i = p, T = u[i][p]; evaluate again.
 *   6. There are exactly *n_moves + 1 evaluations; T rises strictly with every move, so the
 *      procedure ends.  Entries and tables from there on are not written.
 *   7. selected = s, *total = T, *covered = its count; cell_score = fold(s); cell_owner = the slot
 *      whose fold raised the cell, in slot order, or PCP_OWNER_ZX120 / PCP_OWNER_NONE (ties keep
 *      the earlier owner).
 * A set no single move improves is "1-exchange optimal"; it need not be the best set (two sensors
 * may have to move together).  PCP_E_INVALID before any launch, nothing written: k outside 1 ..
 * PCP_PLACE_MAX, n_locked outside 0 .. k, max_moves outside 0 .. PCP_REFINE_MAX_MOVES, reserved
 * != 0, a start index >= n or listed twice, n > PCP_PAIR_MAX_POSES, a step table past
 * PCP_MAX_STEPS, a null required pointer (everything not marked nullable; the move arrays may be
 * null when max_moves == 0), a null context.  No cells: PCP_OK, selected = start, totals and
 * counts 0, no moves, *converged = 1.  One synchronisation; deterministic (two calls give
 * identical bytes); the caller's GridCell flags are neither read nor written; the call's scratch
 * is its own, so the other queries on the context are unchanged by it. */
#define PCP_REFINE_MAX_MOVES 64
typedef struct pcp_refine_params {
    int32_t k;                       /* sensors in the set, 1 .. PCP_PLACE_MAX */
    int32_t n_locked;                /* slots 0 .. n_locked - 1 never move, 0 .. k */
    int32_t max_moves;               /* 0 .. PCP_REFINE_MAX_MOVES */
    int32_t reserved;                /* 0 */
    double  min_separation;          /* metres in XY; <= 0: no constraint */
    int64_t start[PCP_PLACE_MAX];    /* distinct indices into poses5, first k used */
} pcp_refine_params;
int pcp_place_refine(pcp_ctx *ctx, const double *poses5, uint64_t n, const double zx120_pose5[5],
                     const pcp_vl_params *p, const pcp_refine_params *rp,
                     int64_t *selected,        /* [k] the refined set                        */
                     double *total, int32_t *covered,
                     double *start_total, int32_t *start_covered,
                     int32_t *move_slot, int64_t *move_from, int64_t *move_to, /* [max_moves] */
                     double *move_total, int32_t *move_covered,                /* [max_moves] */
                     double *swap_totals,      /* nullable [max_moves + 1][k][n]             */
                     double *cell_score, int32_t *cell_owner,   /* nullable [n_cells] */
                     int32_t *n_moves, int32_t *converged);

/* Kernel timing of pcp_place_refine (the timing tool only): the query's setup (the scoring, the
 * clamped rows, the start total) once, then `reps` repetitions of the start set's evaluation --
 * preparation and evaluation launches, the last block's selection included, nothing committed --
 * between two stream events; *ms_per_eval = the interval / reps.  n >= 1, cells present. */
int pcp_place_refine_burst(pcp_ctx *ctx, const double *poses5, uint64_t n, const double zx120_pose5[5],
                           const pcp_vl_params *p, const pcp_refine_params *rp, int reps,
                           double *ms_per_eval);

/* Greedy placement of mobile sensors with a limited field of view: where to stand and which way
 * to look.  Every pose is searched with every aim of a table; a sensor sees a cell when the cell
 * lies inside its horizontal sector (h_fov about the pose's yaw plus the aim's offset) and inside
 * its elevation band (v_fov about the aim's pitch).  S[p][c] and Z[c] are the values
 * pcp_score_matrix returns for the same arguments with every pose's pitch replaced by 0.0
 * (zx120_pose5 as given): range, visibility and score, nothing else.  max(a, b), osum(v), the
 * separation expression and the first-maximum rule are pcp_place_sensors'.
 *   Host tables (cos, sin, tan: the host C library's double functions): cyp = cos(yaw_p), syp =
 *      sin(yaw_p), yaw_p = poses5[5 p + 4]; ca = cos(aims[2 a]), sa = sin(aims[2 a]); ch =
 *      cos(h_fov * 0.5); lo_a = aims[2 a + 1] - v_fov * 0.5, hi_a = aims[2 a + 1] + v_fov * 0.5;
 *      tlo_a = lo_a <= -M_PI_2 ? -inf : tan(lo_a), thi_a = hi_a >= M_PI_2 ? +inf : tan(hi_a).
 *   Per (p, a, c), in double, every product, sum and sqrt rounded on its own: dx = cx - px, dy =
 *      cy - py, dz = cz - pz; hyp = sqrt(dx * dx + dy * dy); Cy = cyp * ca - syp * sa, Sy = syp *
 *      ca + cyp * sa; fwd = dx * Cy + dy * Sy; H = (h_fov >= 2 pi) || (fwd >= ch * hyp); V =
 *      !(dz < tlo_a * hyp) && !(dz > thi_a * hyp) (negated, so -+inf * 0 = NaN counts as inside:
 *      a cell straight below is in view exactly when the lower bound reaches -90 degrees);
 *      W[p][a][c] = (H && V) ? S[p][c] : +0.0.
 *   1. base = Z, owner[c] = Z[c] > 0 ? PCP_OWNER_ZX120 : PCP_OWNER_NONE; then W[fixed_pose[i]]
 *      [fixed_aim[i]] folded in by max in list order, fixed sensor i owning the cells it raises
 *      (ties keep the earlier owner).  *base_total = osum(base), *base_covered = #{base > 0}.
 *   2. A pose is alive unless it is fixed or, with min_separation > 0, closer than it to a fixed
 *      pose.
 *   3. Round r = 0 .. k_max - 1: t[p][a] = osum(max(base, W[p][a])) for the alive p, -inf for the
 *      others; round_totals[r] holds the whole [n][n_aims] table.
 *   4. (b, ab) = the first maximum in row-major order (pose ascending, then aim; strict '>' from
 *      -inf).
 *   5. Stop when no pose is alive, or unless t[b][ab] > T (T = *base_total, then the last
 *      total_after).
 *   6. selected[r] = b, selected_aim[r] = ab, total_after[r] = T = t[b][ab], covered_after[r] its
 *      count of positive elements; every cell with base[c] < W[b][ab][c] gets owner n_fixed + r,
 *      base = max(base, W[b][ab]); pose b leaves the search, and with min_separation > 0 so does
 *      every pose closer to it than that.
 *   7. cell_score = base, *n_selected = rounds recorded; entries and tables from there on are not
 *      written.
 * PCP_E_INVALID before any launch, nothing written: k_max outside 1 .. PCP_PLACE_MAX, n_aims
 * outside 1 .. PCP_AIM_MAX, n_fixed outside 0 .. PCP_PLACE_MAX, reserved != 0, h_fov not finite or
 * <= 0, v_fov outside (0, pi], a non-finite aim or an aim pitch outside [-pi / 2, pi / 2], n >
 * PCP_PAIR_MAX_POSES, n * n_aims > PCP_AIM_MAX_ROWS, a fixed pose >= n or listed twice, a fixed aim
 * outside the table, a step table past PCP_MAX_STEPS, a null required pointer (everything not
 * marked nullable), a null context.  n == 0 or no cells: PCP_OK, *n_selected = 0, the base totals
 * as defined (0 without cells).  One synchronisation; deterministic (two calls give identical
 * bytes); the caller's GridCell flags are neither read nor written; the call's scratch is its own,
 * so the other queries on the context are unchanged by it. */
#define PCP_AIM_MAX       64      /* aims per call */
#define PCP_AIM_MAX_ROWS  65536   /* n * n_aims */
typedef struct pcp_aim_params {
    int32_t k_max;          /* sensors to place, 1 .. PCP_PLACE_MAX */
    int32_t n_aims;         /* 1 .. PCP_AIM_MAX */
    int32_t n_fixed;        /* aimed sensors already placed, 0 .. PCP_PLACE_MAX */
    int32_t reserved;       /* 0 */
    double  h_fov, v_fov;   /* full angles, radians: h_fov > 0 (>= 2 pi: no horizontal test), 0 < v_fov <= pi */
    double  min_separation; /* metres in XY; <= 0: none */
    int64_t fixed_pose[PCP_PLACE_MAX];   /* indices into poses5, first n_fixed used */
    int32_t fixed_aim[PCP_PLACE_MAX];    /* indices into aims, first n_fixed used */
} pcp_aim_params;
int pcp_place_aimed(pcp_ctx *ctx, const double *poses5, uint64_t n, const double zx120_pose5[5],
                    const pcp_vl_params *p, const pcp_aim_params *ap,
                    const double *aims,        /* [n_aims][2]: yaw offset, pitch (radians) */
                    int64_t *selected, int32_t *selected_aim,        /* [k_max] */
                    double *total_after, int32_t *covered_after,     /* [k_max] */
                    double *round_totals,      /* nullable [k_max][n][n_aims] */
                    double *cell_score, int32_t *cell_owner,         /* nullable [n_cells] */
                    double *base_total, int32_t *base_covered, int32_t *n_selected);

/* Kernel timing of pcp_place_aimed (the timing tool only): the query's setup (the scoring, the
 * tables, the base) once, then `reps` repetitions of round 0's launch -- every row's total, the
 * last block's selection, nothing committed -- between two stream events; *ms_per_round = the
 * interval / reps.  n >= 1, cells present. */
int pcp_place_aimed_burst(pcp_ctx *ctx, const double *poses5, uint64_t n,
                          const double zx120_pose5[5], const pcp_vl_params *p,
                          const pcp_aim_params *ap, const double *aims, int reps,
                          double *ms_per_round);

/* Dense ray fan (BASELINE configs[1]): per pose, n_az x n_el rays, ray (i, j) with local
 * direction (cos e_j cos a_i, cos e_j sin a_i, sin e_j), a_i = 2*pi*i/n_az,
 * e_j = el_min + (el_max-el_min)*(j+0.5)/n_el, rotated by the pose yaw, marched with
 * checkVisibilityWithRaycasting's rule (:765-797) to end = max_distance - 0.08.
 * blocked[p]: rays that hit terrain (occlusion score); units[p] (nullable): sample
 * queries the reference would execute; first_hit (nullable, [p][j][i] int16): sample
 * index of the first blocked sample or -1 (depth = pcp_step_table[k]);
 * best_idx (nullable): argmin blocked, ties -> lowest index. */
typedef struct pcp_fan_params {
    int32_t n_az, n_el;
    double el_min, el_max;     /* radians */
    double max_distance;
} pcp_fan_params;
int pcp_raycast_fan(pcp_ctx *ctx, const double *poses5, uint64_t n, const pcp_fan_params *fan,
                    uint32_t *blocked, uint64_t *units, int16_t *first_hit, int64_t *best_idx);

/* Diagnostic build of the same march (not for timing): stats[0] = samples probed after the
 * exact clip, stats[1] = samples whose 2x2x2 stencil survives the z-band probe and is scanned,
 * stats[2] = point records loaded (12 B each), stats[3] = block directory entries loaded.
 * Over the split fine records stats[1] counts the walk starts actually loaded (a candidate that
 * its window's pivot settles loads none, DESIGN.md section 5 Skip 6) and stats[2] every exact
 * point test, the pivot tests included: stats[0] + stats[1] + stats[2] is the launch's gather
 * lane-load count.  Used to state the roofline's requested bytes. */
int pcp_raycast_fan_stats(pcp_ctx *ctx, const double *poses5, uint64_t n,
                          const pcp_fan_params *fan, uint64_t stats[4]);

/* Kernel timing for the roofline: the production fan kernel of this query, `reps` launches
 * back-to-back between two stream events (after the query's own setup); *ms_per_launch = the
 * interval / reps.  The queue does not idle inside the interval, so the figure agrees with a
 * rocprofv3 kernel trace (a synchronous query's own events also hold the queue wake-up). */
int pcp_raycast_fan_burst(pcp_ctx *ctx, const double *poses5, uint64_t n,
                          const pcp_fan_params *fan, int reps, double *ms_per_launch);

/* The simulated scans of up to PCP_SCAN_MAX_POSES LiDAR poses: pcp_raycast_fan's fan, every
 * blocked ray resolved to the terrain point that stopped it.  N = the input point count of the
 * cloud the current terrain index was built from (the last non-empty pcp_set_terrain, non-finite
 * points included: they are in no index and are never hit; 0 without an index).
 * For pose p and ray id ray = j * n_az + i:  k = first_hit[p][j][i] as pcp_raycast_fan reports
 * it (the same march); k < 0: no return.  Otherwise q = (float(px + dx s_k), float(py + dy s_k),
 * float(pz + dz s_k)) with s_k the step table entry and (dx, dy, dz) = (cy lx - sy ly,
 * sy lx + cy ly, lz) the march's doubles (no contraction); the candidates are the points with
 * acc < r2, acc = ((0 + d0 d0) + d1 d1) + d2 d2 in float, d = q - point, r2 =
 * float((0.08 * 0.7)^2) -- the set that made sample k blocked, never empty; the hit point is the
 * candidate of smallest acc, ties to the lowest input index; range = (float)sqrt((ex ex + ey ey)
 * + ez ez), e = (double)point - pose xyz, in double, every operation rounded.
 *   returns        the blocked rays of pose 0 in ascending ray id, then pose 1's, ...: x, y, z
 *                  the hit point's own bits (map frame), its range, the ray id, the point's input
 *                  index.  At most returns_cap records are written.
 *   offsets        [n + 1]: offsets[p] = where pose p's returns start, offsets[n] = the total =
 *                  *n_returns (a pose without a blocked ray has an empty segment)
 *   hit_point      nullable int32 [n][n_el][n_az]: the hit point's input index, or -1
 *   range_img      nullable float, same shape: the range, or -1.0f
 *   first_hit      nullable, as pcp_raycast_fan's
 *   point_mask     nullable uint64 [N] (mask_cap entries available): bit p set iff some ray of
 *                  pose p resolved to that point; every other bit and the entries of non-finite
 *                  points are zero.  *n_points (nullable) = N.
 *   seen_points    nullable uint32 [n]: points with bit p set
 *   n_seen_any     nullable: points with any bit set (the other points are the blind spots)
 * PCP_E_INVALID before any launch (nothing written) for n > PCP_SCAN_MAX_POSES and for what
 * pcp_raycast_fan rejects (fan dimensions, a step table past PCP_MAX_STEPS).  PCP_E_CAPACITY when
 * returns_cap < the total or (point_mask given) mask_cap < N: *n_returns, *n_points, offsets, the
 * counts and the dense per-ray outputs are valid, no record is written past returns_cap.
 * n == 0: PCP_OK, *n_returns = 0, offsets[0] = 0, the mask all zero.  Deterministic: two calls
 * give identical bytes.  One host synchronisation per call; the caller's GridCell flags and the
 * other queries' device buffers are not touched. */
#define PCP_SCAN_MAX_POSES 64
typedef struct pcp_scan_return {
    float x, y, z;       /* the hit terrain point (its own bits) */
    float range;         /* metres from the pose */
    uint32_t ray;        /* j * n_az + i */
    uint32_t point;      /* input index of the hit point in the terrain cloud */
} pcp_scan_return;
int pcp_simulate_scan(pcp_ctx *ctx, const double *poses5, uint64_t n, const pcp_fan_params *fan,
                      pcp_scan_return *returns, uint64_t returns_cap, uint64_t *n_returns,
                      uint64_t *offsets, int32_t *hit_point, float *range_img,
                      int16_t *first_hit, uint64_t *point_mask, uint64_t mask_cap,
                      uint64_t *n_points, uint32_t *seen_points, uint64_t *n_seen_any);

/* Kernel timing of pcp_simulate_scan (the timing tool only): ms[0] = the query's production fan
 * kernel per launch (`reps` launches between two stream events, as pcp_raycast_fan_burst),
 * ms[1] = its resolve phase -- clears, wave-base scan, k_scan_resolve (records and mask, no dense
 * images), mask counts -- per repetition, `reps` repetitions between two events.  n >= 1. */
int pcp_simulate_scan_burst(pcp_ctx *ctx, const double *poses5, uint64_t n,
                            const pcp_fan_params *fan, int reps, double ms[2]);

/* The fan and the simulated scan of tilted mounts, with an optional beam table.
 * poses6: x, y, z, roll, pitch, yaw per sensor (radians).  pitch has the sign of poses5's pitch:
 * the elevation of the boresight, so negative looks down.  A tf static transform
 * "x y z yaw pitch_tf roll" is pitch = -pitch_tf (the zx120 Velodyne: pitch = -0.4363).
 * For ray (i, j) the local direction is l = (ce_j ca_i, ce_j sa_i, se_j): ca, sa as
 * pcp_raycast_fan's; with el_table (nullable, [fan->n_el] radians, any order) ce_j =
 * cos(el_table[j]), se_j = sin(el_table[j]) and fan->el_min / el_max are not read, without it
 * the fan's uniform table.  Every cos / sin -- the tables', roll's, pitch's, yaw's -- is the host
 * C library's double function.  Then three plane rotations in double, every product and sum
 * rounded on its own (no contraction):
 *   x1 = lx               y1 = ly*cr - lz*sr    z1 = ly*sr + lz*cr    (roll about the boresight)
 *   x2 = x1*cp - z1*sp    y2 = y1               z2 = x1*sp + z1*cp    (pitch: (1,0,0) -> (cp,0,sp))
 *   dx = cy*x2 - sy*y2    dy = sy*x2 + cy*y2    dz = z2               (yaw, as pcp_raycast_fan)
 * Everything after the direction is pcp_raycast_fan's / pcp_simulate_scan's definition word for
 * word: the step table, q = float(p + d s_k), the strict float r2 predicate, first_hit, blocked,
 * units, best_idx, and for the scan the hit point, range, records, offsets, dense images, mask
 * and counts.  With roll = pitch = 0 the direction equals the level fan's as a value (a component
 * can differ in the sign of a zero only), so every output equals the level call's.
 * Limits and errors are the level calls'; in addition a non-finite el_table entry is
 * PCP_E_INVALID before any launch, nothing written.  One host synchronisation per call,
 * deterministic; the caller's GridCell flags and the other queries' buffers are not touched.
 * The launch is timed under PCP_K_RAYCAST_FAN.  Not offered: the multi-GPU and all-reduce forms,
 * the diagnostic modes, an azimuth sector, several beam models in one call. */
int pcp_raycast_fan_mounted(pcp_ctx *ctx, const double *poses6, uint64_t n,
                            const pcp_fan_params *fan, const double *el_table, uint32_t *blocked,
                            uint64_t *units, int16_t *first_hit, int64_t *best_idx);
int pcp_simulate_scan_mounted(pcp_ctx *ctx, const double *poses6, uint64_t n,
                              const pcp_fan_params *fan, const double *el_table,
                              pcp_scan_return *returns, uint64_t returns_cap, uint64_t *n_returns,
                              uint64_t *offsets, int32_t *hit_point, float *range_img,
                              int16_t *first_hit, uint64_t *point_mask, uint64_t mask_cap,
                              uint64_t *n_points, uint32_t *seen_points, uint64_t *n_seen_any);
/* Kernel timing (the timing tool only): as pcp_raycast_fan_burst / pcp_simulate_scan_burst, of
 * the mounted query's production launch and resolve phase. */
int pcp_raycast_fan_mounted_burst(pcp_ctx *ctx, const double *poses6, uint64_t n,
                                  const pcp_fan_params *fan, const double *el_table, int reps,
                                  double *ms_per_launch);
int pcp_simulate_scan_mounted_burst(pcp_ctx *ctx, const double *poses6, uint64_t n,
                                    const pcp_fan_params *fan, const double *el_table, int reps,
                                    double ms[2]);

/* Placement by the terrain the scans reach: greedy maximum coverage over simulated scans, wholly
 * on the device.
 * N = pcp_simulate_scan's N (the input point count of the cloud the current terrain index was
 * built from; 0 without an index).  seen(p) = the set of input indices pcp_simulate_scan reports
 * as hit_point[p][j][i] >= 0 for the same pose and fan (the mounted twin: what
 * pcp_simulate_scan_mounted reports for the same poses6 row and beam table) -- the march, the
 * query point, the float accumulator and the lowest-index tie rule are the scan's.  R = the
 * region of interest: {0 .. N-1} with roi NULL, else {i : roi[i] != 0}; *roi_points = |R|.  The
 * separation expression and the first-maximum rule are pcp_place_sensors', applied to columns 0
 * and 1 of the pose rows.
 *   1. need = R.  For i = 0 .. n_fixed-1 in list order: the points of seen(fixed[i]) in need get
 *      owner i and leave need.  *base_covered = |R| - |need|.  A pose is alive unless it is fixed
 *      or (min_separation > 0) closer than the separation to a fixed pose.
 *   2. Round r = 0 .. k_max-1: stop when no pose is alive; g[p] = |seen(p) & need| for the alive
 *      p; round_gains[r][p] = g[p], -1 for the others; b = the first maximum (the lowest index
 *      among the largest g); stop unless g[b] > 0.
 *   3. selected[r] = b, gain[r] = g[b], covered_after[r] = base_covered + gain[0] + .. + gain[r];
 *      the points of seen(b) in need get owner n_fixed + r and leave need; b leaves the search
 *      and, with min_separation > 0, so does every pose closer to b than the separation.
 *   4. *n_selected = rounds recorded (entries and rows from there on are not written).
 *      point_owner[i] = the owner, or PCP_OWNER_NONE for the points of R nobody reaches and for
 *      every point outside R: the blind spots of the answer are R and owner == NONE.
 *      seen_points[p] = |seen(p)| over all N points (pcp_simulate_scan's seen_points[p]).
 *      *n_points = N.
 * PCP_E_INVALID before any launch, nothing written: what pcp_raycast_fan / _mounted refuse (fan
 * dimensions, a step table past PCP_MAX_STEPS, a non-finite el_table entry), n >
 * PCP_COVER_MAX_POSES or n * n_az * n_el > 2^31, k_max outside 1 .. PCP_PLACE_MAX, n_fixed
 * outside 0 .. PCP_PLACE_MAX, reserved != 0, a fixed index >= n or listed twice, roi given with
 * roi_n != N, a null required pointer (everything not marked nullable), a null context.
 * PCP_E_CAPACITY before any launch when point_owner is given with owner_cap < N: *n_points = N is
 * set and nothing else is written.  n == 0 or N == 0: PCP_OK, *n_selected = 0, *base_covered = 0,
 * *roi_points as defined.
 * One host synchronisation per call; deterministic (two calls give identical bytes); the caller's
 * GridCell flags and the other queries' device buffers are not touched (the call's scratch is its
 * own).  The fan launch is timed under PCP_K_RAYCAST_FAN, the rounds under PCP_K_PLACE. */
#define PCP_COVER_MAX_POSES 1024
typedef struct pcp_cover_params {
    int32_t k_max;          /* sensors to place, 1 .. PCP_PLACE_MAX */
    int32_t n_fixed;        /* sensors already placed, 0 .. PCP_PLACE_MAX */
    int32_t reserved[2];    /* 0 */
    double  min_separation; /* metres in XY; <= 0: none */
    int64_t fixed[PCP_PLACE_MAX];   /* indices into the poses, first n_fixed used */
} pcp_cover_params;
int pcp_place_coverage(pcp_ctx *ctx, const double *poses5, uint64_t n, const pcp_fan_params *fan,
                       const pcp_cover_params *cp,
                       const uint8_t *roi, uint64_t roi_n,       /* nullable; [N], non-zero = counts */
                       int64_t *selected,                        /* [k_max] */
                       uint64_t *gain, uint64_t *covered_after,  /* [k_max] */
                       int64_t *round_gains,                     /* nullable [k_max][n], -1: not alive */
                       uint32_t *seen_points,                    /* nullable [n] */
                       int32_t *point_owner, uint64_t owner_cap, /* nullable [N] */
                       uint64_t *n_points, uint64_t *roi_points, uint64_t *base_covered,
                       int32_t *n_selected);
int pcp_place_coverage_mounted(pcp_ctx *ctx, const double *poses6, uint64_t n,
                               const pcp_fan_params *fan, const double *el_table,
                               const pcp_cover_params *cp, const uint8_t *roi, uint64_t roi_n,
                               int64_t *selected, uint64_t *gain, uint64_t *covered_after,
                               int64_t *round_gains, uint32_t *seen_points, int32_t *point_owner,
                               uint64_t owner_cap, uint64_t *n_points, uint64_t *roi_points,
                               uint64_t *base_covered, int32_t *n_selected);
/* Kernel timing of pcp_place_coverage (the timing tool only): ms[0] = the query's production fan
 * kernel per launch (as pcp_simulate_scan_burst), ms[1] = clear, resolve into the bitsets and
 * counts per repetition, ms[2] = round 0's gain launch with the selection and nothing committed,
 * per repetition; `reps` repetitions between two events each.  n >= 1, a terrain index present. */
int pcp_place_coverage_burst(pcp_ctx *ctx, const double *poses5, uint64_t n,
                             const pcp_fan_params *fan, const pcp_cover_params *cp,
                             const uint8_t *roi, uint64_t roi_n, int reps, double ms[3]);
int pcp_place_coverage_mounted_burst(pcp_ctx *ctx, const double *poses6, uint64_t n,
                                     const pcp_fan_params *fan, const double *el_table,
                                     const pcp_cover_params *cp, const uint8_t *roi,
                                     uint64_t roi_n, int reps, double ms[3]);

/* The exact best pair of mobile sensors by the terrain their scans reach: every pair of the poses
 * evaluated on the device (greedy's two need not be the best two, and the
 * best pair need not hold the best single pose).  N, seen(p), R, the separation expression and the
 * first-maximum rule (strict '>', the lowest index wins) are pcp_place_coverage's; pp is
 * pcp_place_pair's struct.
 *   1. need0 = R minus the points of seen(fixed[i]), i = 0 .. n_fixed-1 in list order; those
 *      points get owner i.  *base_covered = |R| - |need0|: pcp_place_coverage's step 1 values for
 *      the same arguments.
 *   2. A pose is admissible unless it is fixed or (min_separation > 0) closer than the
 *      separation to a fixed pose.
 *   3. g[p] = |seen(p) & need0|; single_gains[p] = g[p] for the admissible p, -1 for the others;
 *      *best_single = the first maximum over the admissible poses, -1 when there is none;
 *      *single_gain its g (0 without one).
 *   4. For a < b, both admissible and (min_separation > 0) not closer to each other than it:
 *      u[a][b] = |(seen(a) | seen(b)) & need0|; pair_gains [n][n] holds u[a][b], every other entry
 *      -1 (the diagonal, the lower triangle, inadmissible pairs); best_pair = the first maximum in
 *      row-major order (a ascending, then b), (-1, -1) when there is no admissible pair;
 *      *pair_gain its u (0 without one).  partner_gain[a] = the first maximum of row a over
 *      b > a and partner[a] = that b, both -1 where row a holds no pair.
 *   5. *n_selected = 2 when a pair exists and *pair_gain > *single_gain; otherwise 1 when a single
 *      exists and *single_gain > 0; otherwise 0.  point_owner describes that answer: the base's
 *      owners, then the chosen pose, or a and then b, folded in that order with owners n_fixed and
 *      n_fixed + 1; PCP_OWNER_NONE for the points of R nobody reaches and for every point
 *      outside R.
 *   6. seen_points, *n_points and *roi_points as pcp_place_coverage's.
 * PCP_E_INVALID before any launch, nothing written: what pcp_place_coverage refuses less k_max
 * (n > PCP_COVER_MAX_POSES included), pp->reserved != 0.  PCP_E_CAPACITY before any launch when
 * point_owner is given with owner_cap < N: *n_points = N is set and nothing else is written.
 * n == 0 or N == 0: PCP_OK, *n_selected = 0, the indices -1 and the gains 0, *base_covered = 0,
 * *roi_points as defined, the tables -1.
 * One host synchronisation per call; deterministic (identical bytes from call to call); counts are
 * integers (32-bit accumulators on the device: N < 2^32).  The caller's GridCell flags and the
 * other queries' device buffers, pcp_place_coverage's included, are not touched (the call's
 * scratch is its own).  The fan launch is timed under PCP_K_RAYCAST_FAN, the pair phase (mask,
 * tiles, selection) under PCP_K_PLACE. */
int pcp_place_coverage_pair(pcp_ctx *ctx, const double *poses5, uint64_t n,
                            const pcp_fan_params *fan, const pcp_pair_params *pp,
                            const uint8_t *roi, uint64_t roi_n,       /* nullable; [N], non-zero = counts */
                            int64_t best_pair[2], uint64_t *pair_gain,
                            int64_t *best_single, uint64_t *single_gain,
                            int64_t *single_gains,                    /* nullable [n], -1: not admissible */
                            int64_t *pair_gains,                      /* nullable [n][n] */
                            int64_t *partner, int64_t *partner_gain,  /* nullable [n] each */
                            uint32_t *seen_points,                    /* nullable [n] */
                            int32_t *point_owner, uint64_t owner_cap, /* nullable [N] */
                            uint64_t *n_points, uint64_t *roi_points, uint64_t *base_covered,
                            int32_t *n_selected);
int pcp_place_coverage_pair_mounted(pcp_ctx *ctx, const double *poses6, uint64_t n,
                                    const pcp_fan_params *fan, const double *el_table,
                                    const pcp_pair_params *pp, const uint8_t *roi, uint64_t roi_n,
                                    int64_t best_pair[2], uint64_t *pair_gain,
                                    int64_t *best_single, uint64_t *single_gain,
                                    int64_t *single_gains, int64_t *pair_gains, int64_t *partner,
                                    int64_t *partner_gain, uint32_t *seen_points,
                                    int32_t *point_owner, uint64_t owner_cap, uint64_t *n_points,
                                    uint64_t *roi_points, uint64_t *base_covered,
                                    int32_t *n_selected);
/* Kernel timing of pcp_place_coverage_pair (the timing tool only): the query's fan, bitsets and
 * fixed sensors once, then ms[0] = the mask pass with the singles per repetition, ms[1] = the pair
 * tiles and the selection (no dense table, nothing committed) per repetition; `reps` repetitions
 * between two events each.  n >= 1, a terrain index present. */
int pcp_place_coverage_pair_burst(pcp_ctx *ctx, const double *poses5, uint64_t n,
                                  const pcp_fan_params *fan, const pcp_pair_params *pp,
                                  const uint8_t *roi, uint64_t roi_n, int reps, double ms[2]);
int pcp_place_coverage_pair_mounted_burst(pcp_ctx *ctx, const double *poses6, uint64_t n,
                                          const pcp_fan_params *fan, const double *el_table,
                                          const pcp_pair_params *pp, const uint8_t *roi,
                                          uint64_t roi_n, int reps, double ms[2]);

/* A set of mobile sensors improved by single-sensor exchanges, scored by the terrain their scans
 * reach, wholly on the device (greedy coverage keeps its bound only without
 * a separation, and a deployment that stands can otherwise only be added to).  N, seen(p), R and
 * *roi_points are pcp_place_coverage's; the separation expression is pcp_place_sensors' strict
 * dx^2 + dy^2 < sep^2 on columns 0 and 1 of the pose rows; the first-maximum rule is strict '>',
 * the lowest index wins; rp is pcp_place_refine's struct, its locked slots in the part of fixed
 * sensors.  C(s) = |(union over j of seen(s_j)) & R|.
 *   1. s = start (rp->start[0 .. k-1]); T = C(s) is *start_covered.
 *   2. One evaluation: for every slot i >= n_locked, L_i = the union of seen(s_j), j != i, and
 *      u[i][p] = |(L_i | seen(p)) & R|; u[i][p] = -1 where the move is inadmissible: slot i is
 *      locked (i < n_locked); p is in s (any slot, i included); or, with min_separation > 0, p is
 *      closer than it to some s_j, j != i.  Only the incoming pose is tested: the start set itself
 *      need not respect the separation.  swap_covered[e] holds evaluation e's whole [k][n] table.
 *   3. The best entry is the first maximum in row-major order (slot ascending, then pose).
 *   4. If it is not > T (or there is none): *converged = 1, stop.  If max_moves moves are recorded
 *      already: stop with *converged = 0.
 *   5. Otherwise move m = (move_slot = i, move_from = s_i, move_to = p, move_covered = u[i][p]);
 *      s_i = p, T = u[i][p]; evaluate again.
 *   6. There are exactly *n_moves + 1 evaluations; T rises strictly with every move, so the
 *      procedure ends.  Entries and tables from there on are not written.
 *   7. selected = s, *covered = T.  slot_unique[i] = the points of R that only slot i of the final
 *      set reaches.  point_owner[i] = the lowest slot whose scan reaches the point, for the points
 *      of R; PCP_OWNER_NONE for the points of R nobody reaches and for every point outside R.
 *      seen_points and *n_points as pcp_place_coverage's.
 * A set no single move improves is "1-exchange optimal"; it need not be the best set.
 * PCP_E_INVALID before any launch, nothing written: what pcp_place_coverage refuses about the fan,
 * the poses, roi_n and null pointers (n > PCP_COVER_MAX_POSES and n * n_az * n_el > 2^31 included);
 * what pcp_place_refine refuses about rp (k outside 1 .. PCP_PLACE_MAX, n_locked outside 0 .. k,
 * max_moves outside 0 .. PCP_REFINE_MAX_MOVES, reserved != 0, a start index >= n or listed twice);
 * a null required pointer (everything not marked nullable; the move arrays may be null when
 * max_moves == 0); a null context.  PCP_E_CAPACITY before any launch when point_owner is given with
 * owner_cap < N: *n_points = N is set and nothing else is written.  N == 0: PCP_OK, selected =
 * start, the counts 0, no moves, *converged = 1; swap_covered and point_owner are not written.
 * One host synchronisation per call (the moves never visit the host); deterministic (identical
 * bytes from call to call); counts are integers (32-bit sums on the device: N < 2^32).  The
 * caller's GridCell flags and the other queries' device buffers, pcp_place_coverage's and
 * pcp_place_coverage_pair's included, are not touched (the call's scratch is its own).  The fan
 * launch is timed under PCP_K_RAYCAST_FAN, the evaluations under PCP_K_PLACE. */
int pcp_place_coverage_refine(pcp_ctx *ctx, const double *poses5, uint64_t n,
                              const pcp_fan_params *fan, const pcp_refine_params *rp,
                              const uint8_t *roi, uint64_t roi_n,       /* nullable; [N], non-zero = counts */
                              int64_t *selected,                        /* [k] the refined set */
                              uint64_t *covered, uint64_t *start_covered,
                              int32_t *move_slot, int64_t *move_from, int64_t *move_to, /* [max_moves] */
                              uint64_t *move_covered,                   /* [max_moves] */
                              int64_t *swap_covered,                    /* nullable [max_moves + 1][k][n], -1: inadmissible */
                              uint64_t *slot_unique,                    /* nullable [k] */
                              uint32_t *seen_points,                    /* nullable [n] */
                              int32_t *point_owner, uint64_t owner_cap, /* nullable [N] */
                              uint64_t *n_points, uint64_t *roi_points, int32_t *n_moves,
                              int32_t *converged);
int pcp_place_coverage_refine_mounted(pcp_ctx *ctx, const double *poses6, uint64_t n,
                                      const pcp_fan_params *fan, const double *el_table,
                                      const pcp_refine_params *rp, const uint8_t *roi,
                                      uint64_t roi_n, int64_t *selected, uint64_t *covered,
                                      uint64_t *start_covered, int32_t *move_slot,
                                      int64_t *move_from, int64_t *move_to, uint64_t *move_covered,
                                      int64_t *swap_covered, uint64_t *slot_unique,
                                      uint32_t *seen_points, int32_t *point_owner,
                                      uint64_t owner_cap, uint64_t *n_points, uint64_t *roi_points,
                                      int32_t *n_moves, int32_t *converged);
/* Kernel timing of pcp_place_coverage_refine (the timing tool only): the query's fan and bitsets
 * once, then ms[0] = the start set's preparation pass (the class rows and their counts) per
 * repetition, ms[1] = its evaluation launch with the selection, nothing committed, per repetition;
 * `reps` repetitions between two events each.  n >= 1, a terrain index present. */
int pcp_place_coverage_refine_burst(pcp_ctx *ctx, const double *poses5, uint64_t n,
                                    const pcp_fan_params *fan, const pcp_refine_params *rp,
                                    const uint8_t *roi, uint64_t roi_n, int reps, double ms[2]);
int pcp_place_coverage_refine_mounted_burst(pcp_ctx *ctx, const double *poses6, uint64_t n,
                                            const pcp_fan_params *fan, const double *el_table,
                                            const pcp_refine_params *rp, const uint8_t *roi,
                                            uint64_t roi_n, int reps, double ms[2]);

/* Greedy coverage placement of sensors with a limited field of view: where to stand and which way
 * to look, scored by the terrain the scans reach.  Every pose is searched
 * with every aim of a table; an aim is a window of the pose's own fan, so the fan is marched and
 * resolved once per pose whatever the aim.  All integers.  N, R, the separation expression and the
 * strict first-maximum rule are pcp_place_coverage's.
 *   w_az in 1 .. n_az (columns), w_el in 1 .. n_el (rings); aims[a] = (az0, el0), 0 <= az0 < n_az,
 *   0 <= el0 <= n_el - w_el.
 *   Window(a) = {(i, j) : ((i - az0_a) mod n_az) < w_az and el0_a <= j < el0_a + w_el}: azimuth
 *      wraps, rings do not.  The window is in the sensor's own (i, j): for a tilted mount an aim
 *      turns the head about its own spin axis.
 *   seen(p, a) = {hit_point[p][j][i] >= 0 : (i, j) in Window(a)}, hit_point as pcp_simulate_scan
 *      reports it for the same pose and fan (the mounted twin: pcp_simulate_scan_mounted for the
 *      same poses6 row and beam table).  A point hit by rays inside and outside a window belongs
 *      to the window; a point hit by several rays of one window counts once.  seen(p) = the union
 *      over the whole fan, pcp_place_coverage's.
 *   1. need = R.  For i = 0 .. n_fixed-1 in list order: the points of seen(fixed_pose[i],
 *      fixed_aim[i]) in need get owner i and leave need.  *base_covered = |R| - |need|.  A pose is
 *      alive unless it is fixed or (min_separation > 0) closer than the separation to a fixed pose.
 *   2. Round r = 0 .. k_max-1: stop when no pose is alive; g[p][a] = |seen(p, a) & need| for every
 *      aim of every alive pose; round_gains[r] holds the whole [n][n_aims] table, -1 in every row
 *      of a pose that is not alive; (b, ab) = the first maximum in row-major order (pose ascending,
 *      then aim); stop unless g[b][ab] > 0.
 *   3. selected[r] = b, selected_aim[r] = ab, gain[r] = g[b][ab], covered_after[r] = base_covered
 *      + gain[0] + .. + gain[r]; the points of seen(b, ab) in need get owner n_fixed + r and leave
 *      need; pose b leaves the search with all its aims and, with min_separation > 0, so does
 *      every pose closer to b than the separation.
 *   4. *n_selected, point_owner, seen_points[p] = |seen(p)|, *n_points and *roi_points as
 *      pcp_place_coverage's.  aim_points[p][a] = |seen(p, a)| over all N points.
 * PCP_E_INVALID before any launch, nothing written: what pcp_place_coverage refuses; n_aims outside
 * 1 .. PCP_COVER_AIM_MAX, n * n_aims > PCP_AIM_MAX_ROWS, w_az outside 1 .. n_az, w_el outside 1 ..
 * n_el, an aim entry out of range, a fixed aim outside the table, a fixed pose >= n or listed
 * twice, reserved != 0, a null required pointer (everything not marked nullable), a null context.
 * PCP_E_CAPACITY and the n == 0 / N == 0 cases as pcp_place_coverage's (aim_points then 0).
 * One host synchronisation per call; deterministic (identical bytes from call to call); the
 * caller's GridCell flags and the other queries' device buffers, pcp_place_coverage's, the pair's
 * and the refine's included, are not touched (the call's scratch is its own).  The fan launch is
 * timed under PCP_K_RAYCAST_FAN, the rounds under PCP_K_PLACE. */
#define PCP_COVER_AIM_MAX 64      /* aims per call (n * n_aims <= PCP_AIM_MAX_ROWS) */
typedef struct pcp_cover_aim_params {
    int32_t k_max;          /* sensors to place, 1 .. PCP_PLACE_MAX */
    int32_t n_aims;         /* 1 .. PCP_COVER_AIM_MAX */
    int32_t n_fixed;        /* aimed sensors already placed, 0 .. PCP_PLACE_MAX */
    int32_t w_az;           /* window width in columns, 1 .. n_az */
    int32_t w_el;           /* window height in rings, 1 .. n_el */
    int32_t reserved[3];    /* 0 */
    double  min_separation; /* metres in XY; <= 0: none */
    int64_t fixed_pose[PCP_PLACE_MAX];   /* indices into the poses, first n_fixed used */
    int32_t fixed_aim[PCP_PLACE_MAX];    /* indices into aims, first n_fixed used */
} pcp_cover_aim_params;
int pcp_place_coverage_aimed(pcp_ctx *ctx, const double *poses5, uint64_t n,
                             const pcp_fan_params *fan, const pcp_cover_aim_params *ap,
                             const int32_t *aims,                      /* [n_aims][2]: az0, el0 */
                             const uint8_t *roi, uint64_t roi_n,       /* nullable; [N], non-zero = counts */
                             int64_t *selected, int32_t *selected_aim, /* [k_max] */
                             uint64_t *gain, uint64_t *covered_after,  /* [k_max] */
                             int64_t *round_gains,                     /* nullable [k_max][n][n_aims], -1: not alive */
                             uint32_t *seen_points,                    /* nullable [n] */
                             uint32_t *aim_points,                     /* nullable [n][n_aims] */
                             int32_t *point_owner, uint64_t owner_cap, /* nullable [N] */
                             uint64_t *n_points, uint64_t *roi_points, uint64_t *base_covered,
                             int32_t *n_selected);
int pcp_place_coverage_aimed_mounted(pcp_ctx *ctx, const double *poses6, uint64_t n,
                                     const pcp_fan_params *fan, const double *el_table,
                                     const pcp_cover_aim_params *ap, const int32_t *aims,
                                     const uint8_t *roi, uint64_t roi_n, int64_t *selected,
                                     int32_t *selected_aim, uint64_t *gain,
                                     uint64_t *covered_after, int64_t *round_gains,
                                     uint32_t *seen_points, uint32_t *aim_points,
                                     int32_t *point_owner, uint64_t owner_cap, uint64_t *n_points,
                                     uint64_t *roi_points, uint64_t *base_covered,
                                     int32_t *n_selected);
/* Kernel timing of pcp_place_coverage_aimed (the timing tool only): ms[0] = the query's production
 * fan kernel per launch, ms[1] = the whole build per repetition (clear, resolve into the bitsets,
 * counts, ranks and the aim masks), ms[2] = round 0's launch with the selection and nothing
 * committed, per repetition; `reps` repetitions between two events each.  n >= 1, a terrain index
 * present. */
int pcp_place_coverage_aimed_burst(pcp_ctx *ctx, const double *poses5, uint64_t n,
                                   const pcp_fan_params *fan, const pcp_cover_aim_params *ap,
                                   const int32_t *aims, const uint8_t *roi, uint64_t roi_n,
                                   int reps, double ms[3]);
int pcp_place_coverage_aimed_mounted_burst(pcp_ctx *ctx, const double *poses6, uint64_t n,
                                           const pcp_fan_params *fan, const double *el_table,
                                           const pcp_cover_aim_params *ap, const int32_t *aims,
                                           const uint8_t *roi, uint64_t roi_n, int reps,
                                           double ms[3]);

/* pcp_place_coverage with a weight per terrain point: a point of the pit's
 * working face may count 200 where a point of the apron counts 1.  N, seen(p), the separation
 * expression, the alive rule, the strict first-maximum rule, the owners, seen_points, the
 * refusals, the capacity rule and the "one host synchronisation, deterministic, other queries'
 * buffers untouched" clauses are pcp_place_coverage's word for word (the call's scratch is its
 * own: pcp_place_coverage's stays as that call leaves it).  What changes:
 *   R = {i : weight[i] != 0};  w(S) = the sum of weight[i] over i in S;  *roi_points = |R|,
 *   *roi_weight = w(R).
 *   1. *base_covered = w(R) - w(need) after the fixed sensors, *base_points = |R| - |need|.
 *   2. g[p] = w(seen(p) & need); round_gains, gain and covered_after are in weight.  Stop unless
 *      g[b] > 0: every weight in need is >= 1, so this is pcp_place_coverage's stop.
 *   3. gain_points[r] = |seen(b) & need| at the moment b is committed.
 *   A non-finite terrain row with a weight counts in *roi_points and *roi_weight and is never
 *   owned.
 * Bounds: a gain is at most 255 N < 2^40 (N < 2^32), exact in the 64-bit gains table and exact as
 * a double in the rounds' first-maximum reduction (< 2^53).
 * Identities: with every weight in {0, 1} every shared output equals pcp_place_coverage's with
 * roi = weight, gain_points == gain and *roi_weight == *roi_points; with every weight in {0, c}
 * the selection is that same one and every weight-valued output is c times it.
 * PCP_E_INVALID before any launch, nothing written: what pcp_place_coverage refuses, weight null,
 * weight_n != N.  n == 0 or N == 0: as pcp_place_coverage, *roi_weight the sum of the weights and
 * *base_points = 0. */
int pcp_place_coverage_weighted(pcp_ctx *ctx, const double *poses5, uint64_t n,
                                const pcp_fan_params *fan, const pcp_cover_params *cp,
                                const uint8_t *weight, uint64_t weight_n,   /* required, [N] */
                                int64_t *selected,                          /* [k_max] */
                                uint64_t *gain, uint64_t *covered_after,    /* [k_max], in weight */
                                uint64_t *gain_points,                      /* nullable [k_max], in points */
                                int64_t *round_gains,          /* nullable [k_max][n], weight, -1: not alive */
                                uint32_t *seen_points,                      /* nullable [n] */
                                int32_t *point_owner, uint64_t owner_cap,   /* nullable [N] */
                                uint64_t *n_points, uint64_t *roi_points, uint64_t *roi_weight,
                                uint64_t *base_covered, uint64_t *base_points,
                                int32_t *n_selected);
int pcp_place_coverage_weighted_mounted(pcp_ctx *ctx, const double *poses6, uint64_t n,
                                        const pcp_fan_params *fan, const double *el_table,
                                        const pcp_cover_params *cp, const uint8_t *weight,
                                        uint64_t weight_n, int64_t *selected, uint64_t *gain,
                                        uint64_t *covered_after, uint64_t *gain_points,
                                        int64_t *round_gains, uint32_t *seen_points,
                                        int32_t *point_owner, uint64_t owner_cap,
                                        uint64_t *n_points, uint64_t *roi_points,
                                        uint64_t *roi_weight, uint64_t *base_covered,
                                        uint64_t *base_points, int32_t *n_selected);
/* Kernel timing of pcp_place_coverage_weighted (the timing tool only): pcp_place_coverage_burst's
 * three phases -- ms[0] the fan, ms[1] the build with the weight planes, ms[2] round 0's gain
 * launch with the selection and nothing committed.  n >= 1, a terrain index present. */
int pcp_place_coverage_weighted_burst(pcp_ctx *ctx, const double *poses5, uint64_t n,
                                      const pcp_fan_params *fan, const pcp_cover_params *cp,
                                      const uint8_t *weight, uint64_t weight_n, int reps,
                                      double ms[3]);
int pcp_place_coverage_weighted_mounted_burst(pcp_ctx *ctx, const double *poses6, uint64_t n,
                                              const pcp_fan_params *fan, const double *el_table,
                                              const pcp_cover_params *cp, const uint8_t *weight,
                                              uint64_t weight_n, int reps, double ms[3]);

/* Diagnostic build with s_memtime stamps (shader clock) per wave: stamps[(p*W + w)*4 + i],
 * W = ceil(n_az*n_el/64), i = 0 start, 1 after direction setup, 2 after the march, 3 end.
 * For locating where wave lifetime goes; never used for timing. */
int pcp_raycast_fan_stamps(pcp_ctx *ctx, const double *poses5, uint64_t n,
                           const pcp_fan_params *fan, uint64_t *stamps);

/* One rank's shard of a pose-sharded fan query whose collective the CALLER runs (one process
 * per GPU: bench.py --gpus N over torch.distributed / RCCL).  The fans of poses5[0 .. n) --
 * global poses [lo, lo + n) of p_total -- are cast as pcp_raycast_fan does, and their keys
 * (blocked << 32) | global pose index are written into the caller's DEVICE buffer
 * keys_dev[p_total] (int64; INT64_MAX in the other ranks' slots), so one all-reduce(MIN) over
 * int64 gives every rank the blocked count of every pose and the argmin (ties: lowest index;
 * virtual_lidar.cpp:467-475).  units_dev (device, nullable, n entries): ray-hit tests per pose.
 * wait_stream (a hipStream_t of the same device, created through the SAME HIP runtime that
 * libpcp links -- not a handle from a framework that bundles its own, such as a PyTorch
 * wheel; nullable): that stream is made to wait for the keys (hipStreamWaitEvent) and the call
 * returns without a host synchronisation; NULL: the call returns once the keys are written.
 * No host copy of the results is made. */
int pcp_raycast_fan_keys(pcp_ctx *ctx, const double *poses5, uint64_t n,
                         const pcp_fan_params *fan, uint64_t lo, uint64_t p_total,
                         int64_t *keys_dev, uint64_t *units_dev, void *wait_stream);

/* ---- one process per GPU: libpcp's own RCCL communicator (bench.py --gpus N) ------------ */
/* The caller's framework only carries the 128-byte id from rank 0 to the others (and its own
 * host-side barriers); the collective runs in this library's HIP runtime on the context's
 * stream, so no stream or device pointer ever crosses into another runtime (a PyTorch wheel
 * bundles its own).  pcp_comm_unique_id: rank 0, before the others' pcp_comm_init_rank
 * (ncclGetUniqueId); pcp_comm_init_rank: ncclCommInitRank on the context's device, collective
 * over all ranks (each rank's context on a distinct device).  The communicator lives until
 * pcp_destroy. */
#define PCP_COMM_ID_BYTES 128
int pcp_comm_unique_id(uint8_t id[PCP_COMM_ID_BYTES]);
int pcp_comm_init_rank(pcp_ctx *ctx, int nranks, const uint8_t id[PCP_COMM_ID_BYTES], int rank);
int pcp_comm_info(const pcp_ctx *ctx, int *nranks, int *rank);   /* 0 ranks: none */
/* Which HIP runtime and RCCL this process's libpcp actually runs on (a PyTorch wheel ships both
 * under the same SONAMEs; whichever was loaded first serves every later NEEDED entry): the
 * versions the libraries report (hipRuntimeGetVersion, ncclGetVersion) and the files they were
 * loaded from (dladdr of hipMalloc / ncclAllReduce).  Paths are NUL-terminated, truncated to
 * cap bytes.  No device call: safe without a GPU. */
typedef struct pcp_runtime_info {
    int32_t hip_runtime_version;   /* HIP_VERSION encoding: major * 10^7 + minor * 10^5 + patch */
    int32_t rccl_version;          /* NCCL_VERSION_CODE encoding: major * 10^4 + minor * 100 + patch */
    char hip_path[512];
    char rccl_path[512];
} pcp_runtime_info;
int pcp_get_runtime_info(pcp_runtime_info *info);
/* One rank's shard of a pose-sharded fan query, collective included (every rank calls it with
 * the same p_total and fan): the fans of poses5[0 .. n) -- global poses [lo, lo + n) -- cast as
 * pcp_raycast_fan does, their keys (blocked << 32) | global pose written into the context's
 * device vector of p_total uint64 (UINT64_MAX elsewhere), ONE ncclAllReduce(ncclUint64,
 * ncclMin) over it on the context's stream, the reduced vector copied back once.
 * blocked_all (host, p_total entries, nullable): every pose's blocked count on every rank;
 * units (host, n entries, nullable): this shard's ray-hit tests per pose; best_idx: the argmin
 * (ties: lowest index; virtual_lidar.cpp:467-475); collective_ms (nullable): the all-reduce's
 * time between two events on the stream.  PCP_E_STATE without a communicator, or when a pose
 * of [0, p_total) was written by no rank.  Replaces the pose loop of runOptimization
 * (virtual_lidar.cpp:467-475) for N processes. */
int pcp_raycast_fan_allreduce(pcp_ctx *ctx, const double *poses5, uint64_t n,
                              const pcp_fan_params *fan, uint64_t lo, uint64_t p_total,
                              uint32_t *blocked_all, uint64_t *units, int64_t *best_idx,
                              double *collective_ms);

/* runOptimization's scoring for one rank of N processes (virtual_lidar.cpp:460-519; every
 * rank calls it with the same p_total, zx120 pose, parameters and cells): this rank's poses5[0 ..
 * n) -- global poses [lo, lo + n) of p_total -- scored as pcp_score_poses scores them, then ONE
 * ncclAllReduce(ncclUint64, ncclMax) on the context's stream over [p_total totals (IEEE bits:
 * totals are >= +0) | p_total covered counts | 3 x n_cells newest-pose flag keys | 1 health
 * word] (the vector pcp_multi_score_poses reduces), then on every rank: the stale GridCell flags
 * resolved from the newest pose overall (:480-519, cell_flags in/out as pcp_score_poses), the
 * strict-'>' argmax over all totals (:471-474) and the colour statistics into *rep.
 * total_all / covered_all (host, p_total entries, nullable): every pose's total and covered
 * count.  collective_ms (nullable): the all-reduce between two events on the stream.
 * A rank whose work before the collective fails still runs it with a poisoned health word: it
 * returns its own error, every other rank PCP_E_STATE (nobody is left blocked in RCCL).
 * PCP_E_STATE too when a pose of [0, p_total) was scored by no rank (cell_flags untouched).
 * Results are identical to pcp_score_poses over all p_total poses on one context. */
int pcp_score_poses_allreduce(pcp_ctx *ctx, const double *poses5, uint64_t n,
                              const double zx120_pose5[5], const pcp_vl_params *p, uint64_t lo,
                              uint64_t p_total, uint8_t *cell_flags, double *total_all,
                              int32_t *covered_all, pcp_vl_report *rep, double *collective_ms);

/* ---- one process, n GPUs: the pose search sharded over devices ------ */
/* pcp_multi_create(n_dev, devices, &m): one context per device (devices NULL: 0 .. n_dev-1)
 * and ONE RCCL communicator over them (ncclCommInitAll).  Poses are partitioned contiguously
 * (rank r takes [r*P/n, (r+1)*P/n), the first P % n ranks one more, the split of
 * runOptimization's candidate loop, virtual_lidar.cpp:467-475); the terrain, zx120 cloud and
 * cells are replicated; each query runs ONE collective:
 *   pcp_multi_raycast_fan  ncclAllReduce(ncclUint64, ncclMin) over P keys (blocked << 32) | p
 *                          -> blocked counts of every pose and the argmin (ties: lowest p)
 *   pcp_multi_score_poses  ncclAllReduce(ncclUint64, ncclMax) over [P totals (IEEE bits of
 *                          values >= +0) | P covered | 3 x n_cells newest-pose flag keys]
 *                          -> the reference's strict-'>' argmax (:471-474) and the stale-flag
 *                          colour statistics (:480-519), as pcp_score_poses.
 * Results are identical to one context over all poses.  The devices must be either all
 * distinct (RCCL) or all the same device (a rehearsal on one GPU: no communicator, the key
 * vectors are combined on that device by a kernel, pcp_multi_info reports uses_rccl = 0); a
 * mixed list such as {0, 0, 1} is refused with PCP_E_INVALID.  The per-device index builds
 * of pcp_multi_set_* run on one host thread per device.  Not thread-safe, like pcp_ctx. */
typedef struct pcp_multi pcp_multi;
int pcp_multi_create(int n_dev, const int *devices, pcp_multi **out);
void pcp_multi_destroy(pcp_multi *m);
const char *pcp_multi_last_error(const pcp_multi *m);
int pcp_multi_info(const pcp_multi *m, int *n_dev, int *uses_rccl);
pcp_ctx *pcp_multi_ctx(pcp_multi *m, int rank);   /* a rank's context (per-rank calls) */
int pcp_multi_set_terrain(pcp_multi *m, const pcp_cloud_view *terrain);
int pcp_multi_set_aux_cloud(pcp_multi *m, const pcp_cloud_view *aux);
int pcp_multi_set_cells(pcp_multi *m, const double *xyz, const float *normals, uint64_t n);
int pcp_multi_raycast_fan(pcp_multi *m, const double *poses5, uint64_t n,
                          const pcp_fan_params *fan, uint32_t *blocked, uint64_t *units,
                          int64_t *best_idx);
int pcp_multi_score_poses(pcp_multi *m, const double *poses5, uint64_t n,
                          const double zx120_pose5[5], const pcp_vl_params *p,
                          uint8_t *cell_flags, double *total_score, int32_t *covered,
                          pcp_vl_report *rep);

/* The longest step table a query may march: max_distance up to about 1,229 m.  pcp_raycast_fan*,
 * pcp_score_poses*, pcp_score_matrix and pcp_generate_and_score return PCP_E_INVALID, before
 * anything is launched, when max_distance - 0.08 gives more samples.  first_hit (int16) would
 * hold 32,767; the bound is lower because the march probes sample k's cell as one float fma
 * A + D k per axis: D's rounding grows with k to ~2e-4 m at k = 4,096 and the probed coordinate's
 * own to ~1e-4 m, together still inside the 1 mm margin of the index's windows that makes a
 * skipped sample a certain miss ("Float probes"); at 32,767 samples they
 * would pass it.  pcp_step_table itself is not bounded by it. */
#define PCP_MAX_STEPS 4096

/* The march's sample distances: s_0 = 0.5, s_{k+1} = s_k + 0.3 (repeated double addition,
 * :765-796) while s_k < end.  Returns the count in *n (writes min(cap, n) values). */
int pcp_step_table(double end, double *steps, uint64_t cap, uint64_t *n);

/* Test infrastructure: the library's device exclusive scan (the index builds' prefix sums)
 * over a host array; out: n + 1 entries (out[n] = the total).  Scans of 2-64 tiles of 2,048
 * run as one look-back pass (PCP_SCAN_ONEPASS, default 1), others as three launches. */
int pcp_debug_exclusive_scan(pcp_ctx *ctx, const uint32_t *in, uint64_t n, uint32_t *out);

/* Test infrastructure: the device's own arithmetic, element by element (one thread per element),
 * through the same device functions the production kernels call (tests/test_device_math_gpu.py).
 * a, b and out are host arrays of n elements of the op's types; b is read only by the ops that
 * name it and aux is written only by PCP_MATH_SCORE_SIN_PART (both may be NULL elsewhere).
 * n == 0 succeeds; a NULL ctx / a / out, a NULL b or aux where the op uses it, and an unknown op
 * give PCP_E_INVALID.
 *   double -> double (pcp_crmath.h; the scoring and the candidate generator):
 *     SCORE_SIN_PART  evaluateCellScore's sin(pi / 2 - acos(a)) as eval_cell computes it;
 *                     aux[i] = 1 when the fast phase decided, 2 when the exact phase did
 *     ACOS_RAW        ocml's acos(a), the composite's first result
 *     ATAN2_RAW       ocml's atan2(a, b), the candidate angles' first result
 *     ATAN2_CR        pcp_cr_atan2_fix(a, b, atan2(a, b)), the candidate generator's expression
 *   float -> float (pcp_libm.h; the PCA normals): ATAN2F (a, b), SINF, COSF, DIVF a / b, SQRTF
 *   bare double operations: F64_DIV a / b, F64_SQRT, F64_TO_F32 (out: float), F64_FMA
 *     fma(a[i], b[2 i], b[2 i + 1]) (b: 2 n doubles), F64_NEXTAFTER nextafter(a, b),
 *     F64_NEARBYINT
 *   NORMAL            a: n float covariances of 9 (row-major 3 x 3), b: n query points of 3,
 *                     out: n float normals of 3 -- computeTerrainNormals' eigen33 and two flips */
#define PCP_MATH_SCORE_SIN_PART 1
#define PCP_MATH_ACOS_RAW 2
#define PCP_MATH_ATAN2_RAW 3
#define PCP_MATH_ATAN2_CR 4
#define PCP_MATH_ATAN2F 10
#define PCP_MATH_SINF 11
#define PCP_MATH_COSF 12
#define PCP_MATH_DIVF 13
#define PCP_MATH_SQRTF 14
#define PCP_MATH_F64_DIV 20
#define PCP_MATH_F64_SQRT 21
#define PCP_MATH_F64_TO_F32 22
#define PCP_MATH_F64_FMA 23
#define PCP_MATH_F64_NEXTAFTER 24
#define PCP_MATH_F64_NEARBYINT 25
#define PCP_MATH_NORMAL 30
int pcp_debug_math(pcp_ctx *ctx, int op, const void *a, const void *b, uint64_t n, void *out,
                   int32_t *aux);

/* Test infrastructure: the terrain's fine-window copy read back exactly as
 * it lies on the device, with every value its build kernels received as a parameter.  Two calls,
 * as elsewhere: with frec, wpts and pts all NULL it fills *geo only (the byte sizes among it);
 * with buffers (each nullable, caps in bytes) it also copies
 *   frec  the record buffer, frec_bytes: tiles, padding records and the split arrays as built
 *         (tile 2: uint16 thresholds, then at start_off the uint32 walk starts; else 8-byte
 *         {start, thresholds} records);
 *   wpts  the entry buffer, wpts_bytes: n_entries entries of 12 (packed: x, y, z) or 16 bytes;
 *   pts   the index's point array, pts_bytes: n_points float4 (x, y, z, original index bits),
 * PCP_E_CAPACITY when a cap is short.  Nothing is de-tiled or unpacked.  geo->built = 0 with
 * PCP_OK when the copy is not built (no terrain, no query yet, or past its caps): the call never
 * builds it, launches nothing, and synchronises the context's stream before its plain copies. */
typedef struct pcp_fine_geo {
    int32_t built;              /* 0: no fine copy; every other field 0 */
    int32_t tile;               /* 0 x-fastest, 1 4 x 4 tiles, 2 split records in 8 x 8 tiles */
    int32_t skip;               /* skip thresholds of the split records' walk start: 1 or 2 */
    int32_t packed;             /* entries of 12 bytes */
    int32_t nx, ny, nz;         /* coarse cells */
    int32_t F, reach, fnx, fny, rz, tsteps;
    uint64_t n_points, n_records, n_entries;
    uint64_t start_off;         /* tile 2: byte offset of the walk-start array in frec */
    uint64_t frec_bytes, wpts_bytes, pts_bytes;
    double ox, oy, oz, c, inv_c, r_q;
    double cf, inv_cf, R2;
    double zq;                  /* threshold step in cells (the float constant, widened) */
    double clear_zt0, clear_c;  /* clearance levels: Zt(iz) = clear_zt0 + iz clear_c */
} pcp_fine_geo;
int pcp_debug_fine_copy(pcp_ctx *ctx, pcp_fine_geo *geo, void *frec, uint64_t frec_cap,
                        void *wpts, uint64_t wpts_cap, void *pts, uint64_t pts_cap);

/* Test infrastructure: the pivot table of the fine-window copy (Skip 6) read
 * back as it lies on the device: one 12-byte (x, y, z) float record per slot of the padded
 * plane of tx x ty tiles of 8 x 8 fine cells, slot of cell (wx, wy) =
 * ((wy / 8) tx + wx / 8) 64 + (wy % 8) 8 + wx % 8.  A cell's record is the point of its window
 * nearest the cell's centre (ox + (wx + 0.5) cf, oy + (wy + 0.5) cf) in xy; an empty window and
 * every padding slot hold (NaN, NaN, -inf).  Two calls as pcp_debug_fine_copy: piv NULL fills
 * *geo only; with a buffer (cap in bytes, PCP_E_CAPACITY when short) it copies the table.
 * geo->built = 0 with PCP_OK when there is no table (no fine copy, or one without split
 * records).  The table does not depend on PCP_FAN_PIVOT (geo->enabled reports the knob).  The
 * call never builds, launches nothing, and synchronises the context's stream before its copy;
 * pcp_debug_fine_copy's output is what it was. */
typedef struct pcp_fine_pivot_geo {
    int32_t built;              /* 0: no table; every other field 0 */
    int32_t enabled;            /* the fan march reads the table (PCP_FAN_PIVOT, default 1) */
    int32_t fnx, fny;           /* fine cells per axis */
    int32_t tx, ty;             /* tiles per axis */
    uint64_t n_slots;           /* tx ty 64 */
    uint64_t bytes;             /* n_slots 12 */
    double ox, oy, cf;
} pcp_fine_pivot_geo;
int pcp_debug_fine_pivot(pcp_ctx *ctx, pcp_fine_pivot_geo *geo, void *piv, uint64_t piv_cap);

/* Test infrastructure: the tight twin of the split records' probe thresholds (DESIGN.md section
 * 5, Skip 7) read back as it lies on the device: one uint16 per record slot, lo | hi << 8, in the
 * layout of the threshold array at the head of pcp_debug_fine_copy's frec (8 x 8 xy tiles, one
 * plane per iz; that call's geometry describes both).  Empty records, with their clearance codes,
 * and padding records equal the specified array's; every other record is never looser than it.
 * *bytes is the array's size, 0 with PCP_OK when there is no twin (no fine copy, one without
 * split records, or the twin's allocation failed); *enabled (may be NULL) reports whether the
 * march reads the twin (PCP_FAN_BAND, default 1) -- the twin does not depend on the knob.  band
 * NULL fills the two values only; with a buffer (cap in bytes, PCP_E_CAPACITY when short) it
 * copies the array.  The call never builds, launches nothing, and synchronises the context's
 * stream before its copy; pcp_debug_fine_copy's output is what it was. */
int pcp_debug_fine_band(pcp_ctx *ctx, uint64_t *bytes, int32_t *enabled, void *band,
                        uint64_t band_cap);

/* diagnostics of the terrain index (cell edge, dims, points) */
typedef struct pcp_index_info {
    uint64_t n_points;
    double cell;
    int32_t nx, ny, nz;
    /* 1: the fine-window copy carries its pivot table (DESIGN.md §5 Skip 6; with fine_tile 2).
       This field sits in what was the padding ahead of bmin: size and offsets are unchanged */
    int32_t fine_pivot;
    double bmin[3], bmax[3];
    /* the layout the terrain scans walk: 0 per-cell runs, 1 2x2x2 block copy, 2 fine-window
       copy (the copies are built at the second query after pcp_set_terrain) */
    int32_t scan_layout;
    /* fine-window record layout (scan_layout 2): 0 x-fastest 8-byte records, 1 4 x 4 tiles of
       them, 2 split records -- 2-byte probe thresholds + 4-byte walk starts, 8 x 8 tiles (this
       field sits in what was the struct's tail padding: the size is unchanged) */
    int32_t fine_tile;
} pcp_index_info;
int pcp_terrain_info(pcp_ctx *ctx, pcp_index_info *info);

#ifdef __cplusplus
}
#endif
#endif /* PCP_ABI_H */
