/*
 * dtsim.h -- C-ABI of libdtsim.so, the MI355X-native batched Duckietown step path.
 *
 * The reference (duckietown/gym-duckietown v6.1.34) has no FFI boundary: its hot
 * path is in-process Python (src/gym_duckietown/simulator.py).  This header is the
 * boundary a maintainer would bind *below* the reference's gym.Env surface; every
 * entry point cites the reference code it replaces (paths under /root/reference/).
 * The ctypes binding is gym-duckietown_amd/dtsim/_ffi.py; INTEGRATION.md shows the
 * stub the reference's simulator.py would add.
 *
 * Conventions
 *   - plain C types, caller-owned inputs (the library copies), no torch types;
 *   - every function returns 0 (DTSIM_OK) or a negative error code and never throws;
 *     dtsim_last_error() returns a thread-local message for the last failure;
 *   - one handle per device; a handle is not thread-safe, distinct handles are
 *     independent; all work is stream-ordered on the handle's HIP stream;
 *   - frames / SoA fields live in device memory owned by the library (or bound by
 *     the caller with dtsim_bind_frames) and are exposed as raw device pointers.
 *   - world frame = the reference's "weird" frame (simulator.py:1629-1652):
 *     x right (tile column i), y up, z = tile row j; heading theta gives
 *     dir = (cos t, 0, -sin t) (simulator.py:2056-2073).
 */
#ifndef DTSIM_H
#define DTSIM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DTSIM_ABI_VERSION 12

/* error codes */
#define DTSIM_OK 0
#define DTSIM_E_INVALID (-1)   /* bad argument */
#define DTSIM_E_HIP (-2)       /* HIP runtime error (message has the hipError string) */
#define DTSIM_E_NOGPU (-3)     /* no HIP device: the library has no CPU fallback */
#define DTSIM_E_STATE (-4)     /* call sequence error (e.g. step before set_maps/reset) */
#define DTSIM_E_LIMIT (-5)     /* a compile-time limit below was exceeded */

/* limits (device tables are LDS-staged) */
#define DTSIM_MAX_MAPS 32
#define DTSIM_MAX_TILES 1024        /* grid_w * grid_h per map */
#define DTSIM_MAX_CURVES 1024       /* per map */
#define DTSIM_MAX_STATIC 56         /* collidable static objects per map */
#define DTSIM_MAX_DYNAMIC 8         /* dynamic objects (DuckieObj + DuckiebotObj) per map */
#define DTSIM_MAX_OBJECTS 64        /* renderable objects per map */
#define DTSIM_MAX_DELAY 16          /* dynamics command delay, in steps (0.15 s: up to 106 Hz) */
#define DTSIM_MAX_TEXTURES 96
#define DTSIM_MAX_MESHES 64

/* dtsim_config.flags */
#define DTSIM_F_RENDER 1u        /* allocate the [N,H,W,3] frame buffer */
#define DTSIM_F_DISTORTION 2u    /* fisheye: needs dtsim_set_distortion_lut (distortion.py:85-125) */
#define DTSIM_F_DOMAIN_RAND 4u   /* per-env camera/light/colour parameters are honoured (simulator.py:551-614) */
#define DTSIM_F_AUTO_RESET 8u    /* envs whose done flag is set restart from the spawn pool at the next step */
#define DTSIM_F_ACTIONS_F64 16u  /* dtsim_step actions are double[...] instead of float[...] */
#define DTSIM_F_PROFILE 32u      /* bracket every kernel launch with HIP events (dtsim_profile_read) */
#define DTSIM_F_LIGHT_CAPTURE 64u /* (ABI v11) device-side resets -- DTSIM_F_AUTO_RESET and dtsim_reset(states = NULL) -- position the new episode's light as GL
                                  * does: reset() calls glLightfv(GL_POSITION) with whatever model-view the LAST FRAME left (simulator.py:565-584), so from the
                                  * second episode on the light given in the init state is taken through the camera of the pose the previous episode ended at
                                  * (a direction is rotated, a position also translated) before it becomes the env's eye-space light.  Honoured by the per-env
                                  * render path (DTSIM_F_DOMAIN_RAND); dtsim_reset(states) takes the light as given (the caller's business, as the gym facade
                                  * does it on the host).
                                  * (ABI v12) With DTSIM_F_DOMAIN_RAND off as well, the shared-camera render lights each env with its own eye-space light
                                  * (colors[12..15] of DTSIM_FIELD_COLORS, whether dtsim_reset(states) set it or a device-side reset captured it); ambient and
                                  * diffuse stay the shared values.  Without this flag the shared camera lights every env with the first episode's light. */

/* dtsim_config.action_mode */
#define DTSIM_ACTION_WHEELS 0    /* Simulator.step: [left, right] duty, clipped to [-1,1] (simulator.py:1669-1672) */
#define DTSIM_ACTION_VEL_STEER 1 /* DuckietownEnv.step: (vel, steering) -> duty (envs/duckietown_env.py:36-61) */

/* done codes (simulator.py:1685-1705 DoneRewardInfo.done_code) */
#define DTSIM_DONE_IN_PROGRESS 0
#define DTSIM_DONE_INVALID_POSE 1
#define DTSIM_DONE_MAX_STEPS 2

/* tile kinds (simulator.py:840-848 + the non-drivable kinds of the map format) */
enum {
  DTSIM_TILE_EMPTY = 0, /* "empty": no tile (simulator.py:820) */
  DTSIM_TILE_STRAIGHT = 1,
  DTSIM_TILE_CURVE_LEFT = 2,
  DTSIM_TILE_CURVE_RIGHT = 3,
  DTSIM_TILE_3WAY_LEFT = 4,
  DTSIM_TILE_3WAY_RIGHT = 5,
  DTSIM_TILE_4WAY = 6,
  DTSIM_TILE_ASPHALT = 7,
  DTSIM_TILE_GRASS = 8,
  DTSIM_TILE_FLOOR = 9,
  DTSIM_TILE_OTHER = 10
};

typedef struct dtsim dtsim_t;

/* Constructor arguments of Simulator / DuckietownEnv that reach the hot path
 * (simulator.py:207-232, envs/duckietown_env.py:15-34). */
typedef struct dtsim_config {
  uint32_t struct_size;  /* sizeof(dtsim_config), ABI check */
  uint32_t flags;        /* DTSIM_F_* */
  int32_t num_envs;
  int32_t device;        /* HIP device ordinal */
  int32_t cam_width;     /* camera_width  (default 640) */
  int32_t cam_height;    /* camera_height (default 480) */
  int32_t frame_skip;    /* simulator.py:1673 */
  int32_t max_steps;     /* simulator.py:1694 */
  int32_t delay_steps;   /* duckietown_world ApplyDelay(0.15 s) in steps; 5 at 30 Hz (PARITY UNPINNED) */
  int32_t action_mode;   /* DTSIM_ACTION_* */
  double delta_time;     /* 1 / frame_rate (simulator.py:300) */
  double robot_speed;    /* constant used by the reward (simulator.py:1702) */
  double gain, trim, radius, k, limit; /* DuckietownEnv kinematics (envs/duckietown_env.py:15) */
  void* stream;          /* hipStream_t to launch on; NULL = library creates one */
} dtsim_config;

/* One world object as interpreted by Simulator.interpret_object (simulator.py:933-1038)
 * and WorldObj.__init__ / DuckieObj.__init__ (objects.py:33-66, 339-365).  OBB corners
 * and SAT axes are computed on the host exactly as the reference does
 * (generate_corners collision.py:64-79, generate_norm collision.py:99-106). */
typedef struct dtsim_object {
  int32_t mesh_id;       /* index into dtsim_set_assets meshes, -1 = not rendered */
  int32_t dynamic;       /* 0 static WorldObj, 1 DuckieObj pedestrian (objects.py:339), 2 DuckiebotObj follower (objects.py:180),
                            3 CheckerboardObj (objects.py:479-587: scripted calibration motion, `vel` carries the initial step counter) */
  int32_t collidable;    /* static && kind != trafficlight (simulator.py:1027-1030) */
  int32_t optional;
  double pos[3];
  double angle;          /* radians */
  double scale;
  double corners[8];     /* [4][2] (x,z) */
  double norm[4];        /* [2][2] */
  double safety_radius;
  double spawn_clear;    /* max(max_coords)*0.5*scale + MIN_SPAWN_OBJ_DIST (simulator.py:1467) */
  /* DuckieObj parameters (objects.py:339-365); ignored for static objects.  For a DuckiebotObj the same
   * four slots carry follow_dist, velocity, gain, trim (objects.py:199-216); its radius / k / limit /
   * wheel_dist / robot_width / robot_length are the reference defaults. */
  double walk_distance, vel, wait_time, wiggle;
  /* TrafficLightObj (objects.py:434-477): every `light_freq` seconds of object time the first material
   * chunk of the mesh (its first `light_tris` triangles) switches between textures light_tex[0] and
   * light_tex[1]; light_pattern is the initial pattern.  light_freq = 0: not a traffic light. */
  int32_t light_freq, light_pattern;
  int32_t light_tex[2];
  int32_t light_tris, light_pad;
} dtsim_object;

typedef struct dtsim_map {
  int32_t grid_w, grid_h;          /* simulator.py:801-802 */
  double tile_size;                /* road_tile_size */
  const uint8_t* tile_kind;        /* [grid_h*grid_w] DTSIM_TILE_*, index j*grid_w+i */
  const uint8_t* tile_angle;       /* [..] 0..3, index into [S,E,N,W] (simulator.py:823-830) */
  const int16_t* tile_tex;         /* [..] texture id (dtsim_set_assets) or -1 */
  const int16_t* tile_curve_off;   /* [..] first curve of the tile, -1 if not drivable */
  const uint8_t* tile_curve_cnt;   /* [..] 2 / 6 / 12 (simulator.py:1151-1335) */
  int32_t n_curves;
  const double* curves;            /* [n_curves][4][2] Bezier control points (x,z) */
  const double* curve_heads;       /* [n_curves][2] chord P3-P0 divided by the tile's Frobenius norm,
                                      computed on the host with the reference's numpy expression
                                      (simulator.py:1355-1356) */
  int32_t n_objects;
  const dtsim_object* objects;     /* [n_objects] in map order */
} dtsim_map;

/* RGBA8 texture, row 0 = v=0 (bottom row of the image, the GL/pyglet origin). */
typedef struct dtsim_texture {
  int32_t width, height;           /* powers of two */
  const uint8_t* rgba;             /* [height][width][4] */
} dtsim_texture;

/* Triangle soup of one mesh after ObjMesh's recentring (objmesh.py:181-232). */
typedef struct dtsim_mesh {
  int32_t n_tris;
  const float* verts;              /* [n_tris][3][3] */
  const float* normals;            /* [n_tris][3][3] */
  const float* colors;             /* [n_tris][3][3] per-vertex Kd */
  const float* uvs;                /* [n_tris][3][2] texture coordinates (objmesh.py:199-207), or NULL */
  const int32_t* tri_tex;          /* [n_tris] texture index of the triangle's material chunk (map_Kd,
                                      objmesh.py:268-275: GL_LINEAR / GL_REPEAT, MODULATE with the lit
                                      vertex colour), -1 = untextured; NULL = all untextured */
} dtsim_mesh;

/* Everything Simulator.reset() decides for one env (simulator.py:528-763).  Drawn on
 * the host in the reference's RNG order (dtsim/reset.py) -- or by the oracle in parity
 * tests -- and uploaded. */
#define DTSIM_MAP_RELOAD 0x40000000

typedef struct dtsim_init_state {
  double pos[3];            /* cur_pos  simulator.py:740 */
  double angle;             /* cur_angle simulator.py:741 */
  int32_t map_id;           /* index into dtsim_set_maps; | DTSIM_MAP_RELOAD: re-create the map's objects even if the env
                               is already on this map (randomize_maps_on_reset reloads the map at every reset,
                               simulator.py:541-544) */
  int32_t dynamics_trim_on; /* dynamics_rand: get_DB18_uncalibrated(trim) simulator.py:746-748 */
  double dynamics_trim;
  double wheel_dist;        /* simulator.py:597 */
  double cam_height;        /* simulator.py:602,612 */
  double cam_angle_deg;     /* simulator.py:605,613 */
  double cam_fov_y_deg;     /* simulator.py:608,614 */
  double camera_noise[3];   /* simulator.py:1768-1769 (applied only with DTSIM_F_DOMAIN_RAND) */
  double horizon_color[3];  /* simulator.py:551-562 */
  double ground_color[3];   /* simulator.py:594 */
  double light_pos[4];      /* simulator.py:565-570, w=0 directional / w=1 positional */
  double light_ambient[3];  /* simulator.py:573-574 */
  double light_diffuse[3];  /* simulator.py:575-576 */
} dtsim_init_state;

/* Result of evaluating the reference's geometry queries at an arbitrary pose. */
typedef struct dtsim_probe {
  int32_t tile_i, tile_j;   /* get_grid_coords simulator.py:1134 */
  int32_t curve_idx;        /* argmax curve of closest_curve_point simulator.py:1362, -1 */
  uint8_t drivable;         /* _drivable_pos(pos) simulator.py:1411 */
  uint8_t collision;        /* _collision(get_agent_corners(pos, angle)) simulator.py:1473 */
  uint8_t valid;            /* _valid_pose(pos, angle, safety_factor) simulator.py:1494 */
  uint8_t in_lane;          /* get_lane_pos2 did not raise NotInLane */
  uint8_t inconvenient;     /* _inconvenient_spawn(pos) simulator.py:1461 */
  uint8_t pad[3];
  double t;                 /* bezier_closest graphics.py:316 */
  double point[2], tangent[2]; /* closest_curve_point (x,z) */
  double dist, dot_dir, angle_deg, angle_rad; /* LanePosition simulator.py:1371-1409 */
  double prox;              /* proximity_penalty2 simulator.py:1430 */
  double reward;            /* compute_reward(pos, angle, robot_speed) simulator.py:1654 */
} dtsim_probe;

/* SoA fields for dtsim_read / dtsim_write / dtsim_field_devptr. */
enum {
  DTSIM_FIELD_POS = 0,        /* double [N][3]  cur_pos */
  DTSIM_FIELD_ANGLE = 1,      /* double [N]     cur_angle */
  DTSIM_FIELD_REWARD = 2,     /* double [N] */
  DTSIM_FIELD_DONE = 3,       /* uint8  [N] */
  DTSIM_FIELD_DONE_CODE = 4,  /* uint8  [N] */
  DTSIM_FIELD_STEP_COUNT = 5, /* int32  [N] */
  DTSIM_FIELD_TILE = 6,       /* int32  [N][2] get_grid_coords(cur_pos) */
  DTSIM_FIELD_LANE = 7,       /* double [N][4] dist, dot_dir, angle_deg, angle_rad (0 if not in lane) */
  DTSIM_FIELD_IN_LANE = 8,    /* uint8  [N] */
  DTSIM_FIELD_PROX = 9,       /* double [N] proximity_penalty2 */
  DTSIM_FIELD_SPEED = 10,     /* double [N] simulator.py:1568 */
  DTSIM_FIELD_TIMESTAMP = 11, /* double [N] */
  DTSIM_FIELD_WHEELS = 12,    /* double [N][2] last [left,right] duty passed to the dynamics */
  DTSIM_FIELD_MAP_ID = 13,    /* int32  [N] */
  DTSIM_FIELD_OBJ_CENTER = 14,/* double [N][DTSIM_MAX_DYNAMIC][2] DuckieObj.center (x,z) */
  DTSIM_FIELD_OBJ_ACTIVE = 15,/* uint8  [N][DTSIM_MAX_DYNAMIC] pedestrian_active */
  DTSIM_FIELD_OBJ_YROT = 16,  /* double [N][DTSIM_MAX_DYNAMIC] y_rot in degrees */
  DTSIM_FIELD_OBJ_PARAMS = 17,/* double [N][DTSIM_MAX_DYNAMIC][3] vel, wait_time, wiggle (write = DR override) */
  DTSIM_FIELD_OBJ_VISIBLE = 18,/* uint8 [N][DTSIM_MAX_OBJECTS] obj.visible (simulator.py:653-656) */
  DTSIM_FIELD_EPISODE = 19,   /* int32  [N] episodes started (auto-reset counter) */
  DTSIM_FIELD_STATE_BLOB = 20,/* opaque: full SoA state, dtsim_state_bytes() bytes (checkpoint) */
  DTSIM_FIELD_OBJ_LIGHT = 21, /* uint8  [N][DTSIM_MAX_OBJECTS] TrafficLightObj.pattern (0 for other objects) */
  DTSIM_FIELD_OBJ_Y = 22,     /* double [N][DTSIM_MAX_DYNAMIC] height of the object centre (CheckerboardObj moves in y) */
  DTSIM_FIELD_OBJ_EXTRA = 23, /* double [N][DTSIM_MAX_DYNAMIC][5] DuckiebotObj follow_dist, radius, wheel_dist, robot_width,
                               * robot_length (objects.py:198-215; its velocity, gain, trim are OBJ_PARAMS) */
  DTSIM_FIELD_CAMERA = 24,    /* float  [N][6]  cam_height, cam_angle[0] (rad), cam_fov_y (rad), camera_noise xyz (simulator.py:596-614) */
  DTSIM_FIELD_COLORS = 25,    /* float  [N][16] horizon rgb, ground rgb, light ambient rgb, diffuse rgb, light_pos xyzw (:551-594) */
  DTSIM_FIELD_WHEEL_DIST = 26,/* double [N]     wheel_dist (:597) */
  DTSIM_FIELD_RENDER_POS = 27,/* int32  [N]     read-only: position of each env in the render order of the last dtsim_render (k_env_sort:
                               * envs standing on the same tile and facing the same way are neighbours; 32 consecutive positions share a
                               * raster workgroup, XCD x owns the x-th eighth of the order); the identity when the pass ran in index order; -1 for the envs a
                               * masked pass (dtsim_render_masked) did not render */
  DTSIM_FIELD_RENDER_PIPE = 28,/* int32 [N]     read-only (ABI v12): the raster of the last dtsim_render, the same value for every env: DTSIM_PIPE_* below,
                               * | DTSIM_PIPE_ENV_LIGHT when the shared camera lit each env with its own light (DTSIM_F_LIGHT_CAPTURE); 0 before any pass.
                               * One value for the whole pass, repeated per env so that the field reads like every other.  The flag
                               * describes the configuration: a segmentation pass is unlit whatever it says. */
  DTSIM_FIELD__COUNT = 29
};

/* DTSIM_FIELD_RENDER_PIPE values */
#define DTSIM_PIPE_GENERIC 1      /* generic raster, shared camera */
#define DTSIM_PIPE_GENERIC_ENV 2  /* generic raster through each env's camera record (domain randomisation, segmentation, per-env light) */
#define DTSIM_PIPE_Q 3            /* quad-record raster, shared camera (tile textures other than 256 x 256, larger grids) */
#define DTSIM_PIPE_V3 4           /* quad-record raster, shared camera, 256 x 256 tile textures */
#define DTSIM_PIPE_V3DR 5         /* quad-record raster, per-env camera (domain randomisation) */
#define DTSIM_PIPE_ENV_LIGHT 16   /* flag: each env lit by its own light on the shared camera */

/* kernels for dtsim_profile_read */
enum { DTSIM_KERNEL_STEP = 0, DTSIM_KERNEL_RENDER = 1, DTSIM_KERNEL_RESET = 2, DTSIM_KERNEL_QUERY = 3, DTSIM_KERNEL_OBSERVE = 4,
       DTSIM_KERNEL_CAMERA_MAPS = 5 /* dtsim_camera_maps' kernel (without its flow set-up launch) */, DTSIM_KERNEL__COUNT = 6 };

int dtsim_abi_version(void);
const char* dtsim_last_error(void);
/* Number of visible HIP devices, or a negative error code. */
int dtsim_device_count(void);

/* Simulator.__init__ (simulator.py:207-384), minus GL. */
int dtsim_create(const dtsim_config* cfg, dtsim_t** out);
void dtsim_destroy(dtsim_t* h);

/* The setters -- dtsim_set_assets, dtsim_set_maps, dtsim_set_distortion_lut(s), dtsim_set_reset_sampler, dtsim_set_spawn_pool,
 * dtsim_set_segment_assets, dtsim_set_label_assets -- and the table caches of dtsim_observe / dtsim_observe_cubic: on failure the handle keeps what it
 * had.  Only what the last render pass left for the post-passes may be dropped: dtsim_draw_leds then waits for a dtsim_render.
 * dtsim_set_maps packs the maps against the assets installed at that moment (texture, mesh and triangle indices), so the order is
 * dtsim_set_assets, then dtsim_set_maps.  A dtsim_set_assets that succeeds while maps are installed releases their render-side
 * tables: physics, reset, query and the reset sampler go on from the maps, and dtsim_render*, dtsim_draw_lines and dtsim_draw_leds
 * return DTSIM_E_STATE until the next dtsim_set_maps. */

/* Textures (graphics.py:69-169 load_texture) and meshes (objmesh.py:62-293). */
int dtsim_set_assets(dtsim_t* h, const dtsim_texture* textures, int n_textures,
                     const dtsim_mesh* meshes, int n_meshes);
/* Simulator._interpret_map output (simulator.py:788-1038), host-prepared. */
int dtsim_set_maps(dtsim_t* h, const dtsim_map* maps, int n_maps);
/* Distortion.rmapx/rmapy (distortion.py:100-111): [cam_height][cam_width] float each.
 * The per-frame cv2.remap(INTER_NEAREST) (distortion.py:118) is folded into the raster. */
int dtsim_set_distortion_lut(dtsim_t* h, const float* rmapx, const float* rmapy);

/* camera_rand (simulator.py:352-358, 611-614, 1968-1970; distortion.py:11-83): every Simulator samples its own K and D
 * once, and its frames are cv2.remap(INTER_NEAREST)-ed through the tables built from them.  Installs n_cal tables
 * src_index[n_cal][cam_height][cam_width] -- per output pixel the rectilinear source pixel (row * cam_width + col, the
 * cvRound of the float maps) or -1 (outside the image: black, BORDER_CONSTANT) -- and the table of each env,
 * env_cal[num_envs] in [0, n_cal).  Needs DTSIM_F_DISTORTION; not with DTSIM_F_LIGHT_CAPTURE.  While installed, the render
 * pass rasterises rectilinear frames into a scratch batch and gathers every (masked) env's frame through its table;
 * dtsim_draw_lines / dtsim_draw_leds refuse (the overlays read the single table), and so do dtsim_depth, dtsim_labels, dtsim_instances and
 * their masked forms unless they are given DTSIM_MAP_ENV_TABLES: with it, the map of env e at camera pixel p is the pass's value at the
 * rectilinear pixel s = src_index[env_cal[e]][p] of that env -- the surface whose colour the gather put at frames[e][p], so map and frame
 * stay pixel-aligned -- and the no-source value (depth 0, DTSIM_LABEL_NONE, DTSIM_INSTANCE_NONE) where s = -1.  n_cal = 0 (tables NULL) uninstalls, and so does dtsim_set_distortion_lut,
 * which installs one table for every env again.  Both copy the tables: the caller's buffers are free on return.
 * DTSIM_LUTS_CAMERA_RAND: device-side resets also scale camera height, angle and fov_y by the randomizer's draws without
 * domain randomisation, and zero the camera noise then (simulator.py:611-614, 1768-1769).  Every call sets this switch from
 * its flags, n_cal = 0 included (camera_rand with one table for every env, e.g. UndistortWrapper's); dtsim_set_distortion_lut
 * leaves it alone. */
#define DTSIM_LUTS_CAMERA_RAND 1u
int dtsim_set_distortion_luts(dtsim_t* h, int n_cal, const int32_t* src_index, const int32_t* env_cal, uint32_t flags);
/* Host-only builders of those tables (no handle, no GPU), bit-identical to dtsim/distortion.py's numpy statement for any
 * K and D, spread over at most 16 threads.  dtsim_build_remap_maps: per calibration K[9] and D[5] (the plumb-bob model)
 * and inv_new_K[9] (np.linalg.inv of the new camera matrix, row-major), the rectify map and its inversion
 * (Distortion._invert_map, distortion.py:138-216): rmapx / rmapy [n_cal][height][width] float, NaN for holes.
 * dtsim_fill_pack_remap: Distortion._fill_holes (distortion.py:218-265) in place, visiting the holes of table i in the
 * order hole_order[hole_off[i] .. hole_off[i + 1]) (row * width + col: the iteration order of the reference's Python set),
 * then, unless src_index is NULL, the packed source index of dtsim_set_distortion_luts. */
int dtsim_build_remap_maps(int width, int height, int n_cal, const double* K, const double* D, const double* inv_new_K,
                           float* rmapx, float* rmapy);
int dtsim_fill_pack_remap(int width, int height, int n_cal, float* rmapx, float* rmapy, const int32_t* hole_order,
                          const int64_t* hole_off, int32_t* src_index);

/* Simulator.reset() for the envs with mask[e] != 0 (mask NULL = all): state taken from
 * states[e] (array of num_envs entries). */
int dtsim_reset(dtsim_t* h, const uint8_t* mask, const dtsim_init_state* states);   /* states == NULL: device sampler */
/* Device-side reset sampler.  The reference's reset() draws, per env, the domain-
 * randomisation values (simulator.py:546-614, randomizer.py:36-91), the visibility of optional objects
 * (:648-656), a start tile (:659-676) and then poses until one is accepted (:692-738: not an
 * inconvenient spawn, valid at safety factor 1.3, within accept_start_angle_deg of the lane).  With a
 * sampler installed the same *distributions* and acceptance test run on the device from a counter-based
 * generator (Philox4x32-10 keyed by seed and env index, counter = episode) -- the stream differs from
 * numpy's PCG64, so this mode is for throughput, not for RNG-order parity (dtsim_reset with host states
 * / the spawn pool keep that).  Used by DTSIM_F_AUTO_RESET when installed (it takes precedence over the
 * pool) and by dtsim_reset(h, mask, NULL). */
typedef struct dtsim_reset_sampler {
  uint64_t seed;
  int32_t domain_rand;              /* draw camera / light / colour / wheel_dist perturbations */
  int32_t dynamics_rand;            /* apply the drawn trim (simulator.py:744-750) */
  int32_t map_cycle;                /* 1: MultiMapEnv, the next map at every reset (multimap_env.py:44-49);
                                       2: randomize_maps_on_reset, a uniformly drawn map, reloaded (simulator.py:541-544) */
  int32_t max_attempts;             /* MAX_SPAWN_ATTEMPTS, 5000 */
  double accept_start_angle_deg;    /* simulator.py:724-728 */
  double color_sky[3], color_ground[3];
  int32_t start_tile[DTSIM_MAX_MAPS][2];  /* user_tile_start / the map's start_tile; -1 = a random drivable tile */
  int32_t has_start_pose[DTSIM_MAX_MAPS]; /* the map defines start_pose: spawn at tile * tile_size + pose, no rejection loop */
  double start_pose[DTSIM_MAX_MAPS][3];   /* (x offset, z offset, angle): simulator.py:679-688 */
} dtsim_reset_sampler;
int dtsim_set_reset_sampler(dtsim_t* h, const dtsim_reset_sampler* sampler);   /* NULL uninstalls */
/* Reset, with the installed sampler, every env whose done flag is set (the mask is read on the device: no
 * host round trip).  What a vectorised learner loop does right after a step: read reward / done, then
 * restart the finished episodes so that the observation it gets is the new episode's first one. */
int dtsim_reset_done(dtsim_t* h);

/* Pool of spawn states used by DTSIM_F_AUTO_RESET: env e starts episode k from
 * pool[(e + k * num_envs) % n_pool]. */
int dtsim_set_spawn_pool(dtsim_t* h, const dtsim_init_state* pool, int n_pool);

/* n_steps x { [DuckietownEnv.step ->] Simulator.step } without the render
 * (simulator.py:1669-1705; update_physics :1551; _update_pos :2076; _compute_done_reward :1685).
 * actions: [n_steps][num_envs][2], float (or double with DTSIM_F_ACTIONS_F64), host or
 * device pointer (actions_on_device).  Asynchronous. */
int dtsim_step(dtsim_t* h, const void* actions, int n_steps, int actions_on_device);

/* dtsim_step with flags; dtsim_step(...) == dtsim_step_ex(..., 0).
 *   DTSIM_STEP_ONE_UPDATE  one `Simulator.update_physics(action)` (simulator.py:1551-1584) per step: like dtsim_step but
 *                          the action is the wheel pair update_physics takes -- no (vel, steering) kinematics
 *                          (DuckietownEnv.step's) and no np.clip (Simulator.step's, :1670) -- and
 *                          frame_skip is not applied (step_count += 1, timestamp += delta_time, speed, every object
 *                          stepped once; reward / done are refreshed for the new state -- they are pure functions of it,
 *                          `_compute_done_reward` :1685 evaluates them on demand in the reference).
 *   DTSIM_STEP_POSE_ONLY   the module-level `_update_pos(self, action)` (simulator.py:2076-2088): the dynamics state
 *                          (incl. the delayed-command queue) advances by one delta_time and the resulting pose is
 *                          written to the pose fields; step_count, timestamp, speed, objects, reward and done are
 *                          left alone, DuckietownEnv's (vel, steering) kinematics and auto-reset do not apply (the
 *                          action is the wheel pair `_update_pos` takes, simulator.py:2083). */
enum { DTSIM_STEP_ONE_UPDATE = 1u, DTSIM_STEP_POSE_ONLY = 2u };
int dtsim_step_ex(dtsim_t* h, const void* actions, int n_steps, int actions_on_device, uint32_t flags);

/* Simulator.render_obs (simulator.py:1953-1972) = _render_img (:1707-1951) + distort:
 * writes [num_envs][cam_height][cam_width][3] uint8, row 0 = image top.  Asynchronous. */
int dtsim_render(dtsim_t* h);

/* Segmentation render, `_render_img(..., segment=True)` (simulator.py:1730-1737, 1753, 1808, 1879; reached from
 * reset(segment) :760, render_obs(segment) :1953 and render(mode, segment) :1974): lighting off, colour buffer
 * cleared to and ground quad drawn in magenta, every texture replaced by its segmented version
 * (graphics.py:52-57 Texture.bind -> load_texture(segment=True) :70-126), every mesh drawn through
 * get_mesh(name, segment=True) = flat `gen_segmentation_color(mesh_name)` modulated by the per-vertex Kd
 * (objmesh.py:255-292, 360-362).  The segmented textures are prepared on the host (dtsim/assets.py) and must
 * mirror the dtsim_set_assets list entry for entry (same count, same sizes); mesh_rgb is [n_meshes][3]. */
int dtsim_set_segment_assets(dtsim_t* h, const dtsim_texture* textures, int n_textures,
                             const uint8_t* mesh_rgb, int n_meshes);
enum { DTSIM_RENDER_SEGMENT = 1u, DTSIM_RENDER_GL_FILTER = 2u };
/* dtsim_render with flags (DTSIM_RENDER_*); dtsim_render(h) == dtsim_render_ex(h, 0).
 * DTSIM_RENDER_GL_FILTER (ABI v11): this pass filters tile textures with the arithmetic of the reference's renderer -- Mesa llvmpipe's 8-bit
 * GL_LINEAR: two lerps with an 8-bit intermediate (csrc/raster_common.h gl_linear_rgb) -- instead of the quad-record kernels' one-pass byte-weight
 * filter: the generic raster runs, 2 - 4 x slower, and the frames are bit-identical to the reference's on 99.2 - 99.96 % of the pixels instead of
 * within +-1/255 on all but 0.25 % (tests/test_gpu_gl_golden.py).  For validation against reference frames, not for throughput. */
int dtsim_render_ex(dtsim_t* h, uint32_t flags);
/* Masked render: dtsim_render_ex(h, flags) for the envs with mask[e] != 0 only.  `mask` is a DEVICE pointer to num_envs bytes (nonzero =
 * selected), read on the handle's stream; the call is asynchronous and never waits for the host, so the count of selected envs is never
 * needed there.  Frames of unselected envs are not written.  The quad-record pipelines (DTSIM_PIPE_V3, DTSIM_PIPE_Q, DTSIM_PIPE_V3DR) sort the
 * selected envs into positions [0, live) of the render order (whatever N), their setup kernels skip the others and their rasters stop at the
 * live count, so the pass costs about the selected fraction of a full one plus a fixed part (the sort, the setup launches, the workgroups
 * past the live chunks leaving at once).  Afterwards DTSIM_FIELD_RENDER_POS reads -1 for the envs that were not rendered, and
 * dtsim_draw_lines / dtsim_draw_leds fail with DTSIM_E_STATE until a full dtsim_render.
 * Fallback: the generic pipelines -- segmentation, DTSIM_RENDER_GL_FILTER, the per-env camera without the quad records, tile textures or
 * tables outside the quad-record limits -- render EVERY env, as dtsim_render_ex would: an unselected env's unchanged state renders to the
 * same bytes, so its frame keeps its content; only the cost differs.  Typical use: after dtsim_step, a full pass renders the frames step()
 * returns, dtsim_copy_rows keeps those of the finished envs, dtsim_reset_done restarts them, and this call renders just their first frames. */
int dtsim_render_masked(dtsim_t* h, uint32_t flags, const uint8_t* mask);
/* GL_LINE overlays of the reference -- draw_curve (simulator.py:1886-1904, graphics.py:336-349) and draw_bbox (simulator.py:1907-1918,
 * objects.py:131-146) -- as a post-pass on the frames the last dtsim_render made: `lines` = [n][9] floats, world-space segment
 * (ax, ay, az, bx, by, bz) + colour (r, g, b in 0..1, the glColor3f of the line); env_idx[i] = the env segment i is drawn into (NULL: all
 * into env 0; must be non-decreasing).  Each segment goes through the env's camera, is clipped at the near plane and rasterised as a
 * 1-pixel line under 4x multisampling (coverage per sample, first line wins a sample); the colour is the glColor lit as a surface with
 * normal +y.  Lines are not depth-tested against mesh objects (they lie above the tile plane).  Synchronous (host segments).
 * Both post-passes (this and dtsim_draw_leds) use the cameras / projected triangles of THE LAST dtsim_render: dtsim_step, dtsim_reset,
 * dtsim_reset_done and dtsim_write invalidate them -- the call then fails with DTSIM_E_STATE until the state has been rendered again. */
int dtsim_draw_lines(dtsim_t* h, const float* lines, const int32_t* env_idx, int n);
/* The LED spheres of enable_leds (objects.py:68-121: per LED of a duckiebot-kind object a 1 cm gluSphere at alpha 1 and a halo at alpha 0.2,
 * additively blended -- glBlendFunc(GL_SRC_ALPHA, GL_ONE) -- with depth test and depth writes, lit, untextured) as a post-pass on the frames
 * the last dtsim_render made: `spheres` = [n][8] floats, world-space centre (x, y, z), radius, glColor (r, g, b in 0..1), alpha, in DRAW
 * ORDER; env_idx as for dtsim_draw_lines.  Per MSAA sample the depth of the opaque scene is recomputed (planes analytically, meshes from
 * the projected triangles the render pass left) and every sphere whose front surface is nearer adds alpha x its lit colour and writes its
 * depth; the pixel becomes frame + sum / 4.  Deviations from the GL result (it depends on gluSphere's strip order): analytic spheres, front
 * surfaces only, all spheres after all opaque objects.  Needs a preceding dtsim_render of the same state (not the segment view).
 * Synchronous (host spheres). */
int dtsim_draw_leds(dtsim_t* h, const float* spheres, const int32_t* env_idx, int n);
void* dtsim_frames_devptr(dtsim_t* h);
size_t dtsim_frames_bytes(const dtsim_t* h);
/* Render into caller-owned device memory instead (e.g. a torch tensor that is the
 * send buffer of the RCCL all-gather). NULL restores the internal buffer. */
int dtsim_bind_frames(dtsim_t* h, void* devptr);
/* The north star's exchange (no counterpart in the reference, which runs one env per process):
 * RCCL all-gather of this rank's uint8 frame batch (the buffer dtsim_frames_devptr / dtsim_bind_frames names) into
 * `recv` = device memory for n_ranks * dtsim_frames_bytes(h) bytes, rank-major, enqueued on the handle's stream behind
 * the last render (stream-ordered: dtsim_sync or the next call on the handle waits for it).  `nccl_comm` is an
 * ncclComm_t the CALLER created (one process per GPU; ncclCommInitRank in C, or the communicator of its framework);
 * librccl.so is resolved with dlopen at the first call -- the library has no link-time dependency on it, and the
 * call fails with DTSIM_E_STATE where it is absent.  `send` = NULL gathers the frame batch; otherwise `send` /
 * `send_bytes` name another device buffer of this rank to gather instead (e.g. the dtsim_observe output: 57.6 KB per
 * env at 160 x 120 instead of 921.6 KB).  ORDERING: the collective is ordered behind earlier work on the HANDLE's stream only.
 * `recv` (and a caller-owned `send`) must be ready on that stream when the call is made -- a buffer another stream is still
 * filling or zeroing must be synchronised first (host wait, or an event the handle's stream waits on: dtsim_stream()); readers on
 * another stream wait for the handle's stream likewise.  dtsim/sharding.py: ShardedSimulator.gather_frames() uses this entry point
 * on RCCL jobs (events both ways, no host wait). */
int dtsim_allgather_frames(dtsim_t* h, void* nccl_comm, void* recv, const void* send, size_t send_bytes);

/* Learner-side observation of the rendered frame batch, on the device (what the reference's learners do
 * per env on the host): ResizeWrapper (learning/utils/wrappers.py:38-54, scipy imresize == PIL
 * Image.resize BILINEAR, reproduced bit-exactly: Pillow's two-pass 22-bit fixed-point resampler with its
 * uint8 intermediate), optionally ImgWrapper (HWC -> CHW, :72-86) and NormalizeWrapper (/ 255 -> float32,
 * :57-69).  `taps_*` are Pillow's per-output-coordinate tables (first tap, tap count / fixed-point taps)
 * as built by dtsim/resample.py; pass NULL tables for an axis whose size does not change.
 * out: device pointer to [num_envs][out_h][out_w][3] (DTSIM_OBS_HWC) or [num_envs][3][out_h][out_w]
 * (DTSIM_OBS_CHW), uint8 or float32 (DTSIM_OBS_F32).  Asynchronous, stream-ordered after dtsim_render.
 * The handle keeps one device copy of the tables, keyed on their contents (and the output size): a call whose
 * tables differ from the cached ones re-validates and re-uploads them, whatever the output size. */
enum { DTSIM_OBS_HWC = 0, DTSIM_OBS_CHW = 1, DTSIM_OBS_F32 = 2 };
int dtsim_observe(dtsim_t* h, void* out, int out_h, int out_w, int flags,
                  const int32_t* bounds_x, const int32_t* taps_x, int ksize_x,
                  const int32_t* bounds_y, const int32_t* taps_y, int ksize_y);

/* The reference's own ResizeWrapper (src/gym_duckietown/wrappers.py:129-138): cv2.resize(obs, (out_w, out_h),
 * interpolation=cv2.INTER_CUBIC) of every frame of the batch, on the device -- OpenCV's 8-bit fixed-point path as
 * published in imgproc/resize.cpp: four taps per axis (A = -0.75) in 11-bit fixed point, replicated borders, int32
 * rows without intermediate rounding, saturate_cast<uchar>((v + 2^21) >> 22).  first_*[i] = source index of the first
 * of the four taps of output coordinate i (may be negative), taps_*: [out][4], both as built by dtsim/resample.py
 * cubic_coeffs (host pointers).  out / flags as dtsim_observe.  Asynchronous, stream-ordered after dtsim_render. */
int dtsim_observe_cubic(dtsim_t* h, void* out, int out_h, int out_w, int flags,
                        const int32_t* first_x, const int32_t* taps_x, const int32_t* first_y, const int32_t* taps_y);
/* dtsim_observe / dtsim_observe_cubic for the envs with mask[e] != 0 only (`mask`: DEVICE pointer to num_envs bytes, nonzero = selected):
 * the rows of selected envs are written exactly as the unmasked call writes them, the rows of the others are left untouched.  The launch
 * is sized for num_envs; the workgroups of unselected envs leave at once.  Asynchronous, stream-ordered. */
int dtsim_observe_masked(dtsim_t* h, void* out, int out_h, int out_w, int flags, const uint8_t* mask,
                         const int32_t* bounds_x, const int32_t* taps_x, int ksize_x,
                         const int32_t* bounds_y, const int32_t* taps_y, int ksize_y);
int dtsim_observe_cubic_masked(dtsim_t* h, void* out, int out_h, int out_w, int flags, const uint8_t* mask,
                               const int32_t* first_x, const int32_t* taps_x, const int32_t* first_y, const int32_t* taps_y);
/* Row e of `src` -> row e of `dst` (row_bytes each, device pointers, num_envs rows) for every env with mask[e] != 0 (DEVICE pointer to
 * num_envs bytes); other rows of dst are left untouched.  16-byte accesses when both pointers and row_bytes are 16-byte aligned.  For the
 * final observations (or frames) of the envs that finished a step, before dtsim_reset_done.  Asynchronous, stream-ordered. */
int dtsim_copy_rows(dtsim_t* h, void* dst, const void* src, size_t row_bytes, const uint8_t* mask);
/* The observation history of every env, kept by the caller on the device (gym's FrameStack, for the whole batch): push this step's
 * observation into a stack of the last `depth` ones.
 *   obs:   DEVICE pointer to [num_envs][3][out_h][out_w] uint8 -- what dtsim_observe* writes with DTSIM_OBS_CHW and without DTSIM_OBS_F32.
 *   stack: DEVICE pointer to [num_envs][depth][C][out_h][out_w], C = 3, or 1 with DTSIM_OBS_GRAY; uint8, or float32 with DTSIM_OBS_F32.
 *          Slot 0 is the oldest.  The caller owns it and the handle keeps no history: the call is stateless.  obs and stack must not overlap.
 *   first, mask: DEVICE pointers to num_envs bytes, or NULL (no env starts anew / every env is selected).
 * For every selected env e: with first[e] != 0 all `depth` slots become the new observation (an episode's first observation is replicated),
 * else slot k takes slot k + 1 for k < depth - 1; the last slot takes the new observation.  The rows of unselected envs keep every byte,
 * whatever `first` says.  The new observation is converted on the way: DTSIM_OBS_GRAY is Pillow's convert("L") of the resized uint8 pixel,
 * (19595 R + 38470 G + 7471 B + 0x8000) >> 16; DTSIM_OBS_F32 stores (float)v / 255.0f as dtsim_observe does, so the newest slot of a colour
 * float32 stack equals dtsim_observe(CHW | F32) of the same frames bit for bit.  depth == 1 is the pure conversion.
 * flags must hold DTSIM_OBS_CHW (there are no HWC stacks) and nothing but DTSIM_OBS_CHW | DTSIM_OBS_F32 | DTSIM_OBS_GRAY; a null handle, stack
 * or obs, depth outside 1 .. DTSIM_OBS_MAX_DEPTH, a non-positive size or such flags return DTSIM_E_INVALID before anything touches a device.
 * In place, 16-byte accesses when the bases and the slot's size in bytes are 16-byte aligned.  Asynchronous, stream-ordered (as dtsim_copy_rows). */
enum { DTSIM_OBS_GRAY = 4 };          /* dtsim_obs_push only */
#define DTSIM_OBS_MAX_DEPTH 16
int dtsim_obs_push(dtsim_t* h, void* stack, const uint8_t* obs, int depth, int out_h, int out_w, int flags,
                   const uint8_t* first, const uint8_t* mask);
/* A weighted sum of several whole frame batches, element by element: the blend of the reference's MotionBlurWrapper
 * (learning/utils/wrappers.py:8-36: np.average of the four frames of a step's sub-updates, weights 0.8 / 0.15 / 0.04 / 0.01, oldest first) in
 * exact integer arithmetic -- the weights as integers w[i] with the sum D, here 80, 15, 4, 1 hundredths.
 *   frames:  HOST array of n DEVICE pointers, each to [num_envs][cam_height][cam_width][3] uint8, oldest first.
 *   weights: HOST array of n integers, each 0 .. 255, with D = sum of them in 1 .. 256: every S = sum of w[i] * frames[i][j] fits 16 bits.
 *            Both arrays are read during the call and passed to the kernel by value.
 *   out:     DEVICE pointer to [num_envs][cam_height][cam_width][3]: uint8 (flags 0), out[j] = (2 S + D) / (2 D) in integer division, i.e. S / D
 *            rounded half up; or float32 (DTSIM_OBS_F32, the only flag), out[j] = (float)S / (float)D, one IEEE division -- for the reference's
 *            weights bit for bit np.float32 of what np.average returns.  A uint8 `out` may be any of frames[i] (every input of an element is
 *            loaded before the element is stored); a float32 `out` must not overlap an input.
 *   mask:    DEVICE pointer to num_envs bytes, or NULL = every env; as dtsim_copy_rows: the rows of unselected envs keep every byte.
 * A null handle, out, frames, weights or frames[i], n outside 1 .. DTSIM_BLEND_MAX, a weight above 255, D outside 1 .. 256 or any other flag
 * return DTSIM_E_INVALID before anything touches a device; a handle without DTSIM_F_RENDER returns DTSIM_E_STATE.  16-byte accesses when every
 * base and the frame size in bytes are 16-byte aligned.  Asynchronous, stream-ordered.
 * DuckietownVecEnv(motion_blur=...) renders a step's sub-updates into a ring of frame batches and blends them with this call.
 * Deviation: the reference hands the float64 average on (its learners' imresize then rescales by the array's min and max); the env rounds the
 * blend half up to uint8 and resizes it like every other frame.  The float32 output is the unrounded value. */
#define DTSIM_BLEND_MAX 8
int dtsim_blend_frames(dtsim_t* h, void* out, const void* const* frames, const uint32_t* weights, int n, int flags, const uint8_t* mask);
/* The depth map of every camera frame, on the device: ground-truth geometry beside the observation (no counterpart in the reference, whose
 * only per-pixel output is the frame).
 * THE QUANTITY.  For camera pixel (r, c) of env e, depth is the smallest, over the four MSAA samples of the frame's SOURCE pixel, of the eye
 * depth of the nearest opaque surface: tile plane, ground quad, mesh triangles.
 *   - The source pixel is (r, c) itself without the fisheye; with it, the pixel the handle's distortion table names for (r, c).
 *   - Eye depth is the t of the eye-space ray (dx, dy, -1) t: distance along the optical axis, not range.
 *   - The samples, their offsets and the near / far limits (0.04 / 100) are those of the colour pass; plane ownership (tile present, ground
 *     extent, sky) is the colour pass's own test, mesh depth that of its z-buffer.
 *   - A pixel whose four samples all see the clear colour has depth +inf.
 *   - A pixel the fisheye leaves without a source (the frame's black border) has depth 0.
 *   - LED spheres and line overlays are not part of it.
 * The minimum (not a vote or a mean): a thin silhouette that colours a pixel also sets its depth, and it is conservative for obstacle distance.
 * SIZE.  out: DEVICE pointer to [num_envs][oh][ow], float32, or IEEE half (round to nearest even, inf stays inf) with DTSIM_DEPTH_F16.  The map
 * is point-sampled, never filtered (depth must not be blended across a silhouette): cam_height % oh == 0 and cam_width % ow == 0, else
 * DTSIM_E_INVALID; with sy = cam_height / oh and sx = cam_width / ow, out[e][i][j] is the depth of camera pixel (i sy + sy / 2, j sx + sx / 2)
 * in integer division -- the small map is full[:, sy/2::sy, sx/2::sx], and only those pixels are traced.
 * STATE.  A post-pass of a render, under the rules of dtsim_draw_leds: it reads the cameras and projected triangles the last pass left, so a
 * colour dtsim_render / dtsim_render_ex (not the segment view) of the CURRENT state must precede it -- dtsim_step, dtsim_reset,
 * dtsim_reset_done, dtsim_write, dtsim_set_maps, dtsim_set_assets and dtsim_set_distortion_lut invalidate -- and per-env distortion tables
 * (dtsim_set_distortion_luts) are refused without DTSIM_MAP_ENV_TABLES; all of these DTSIM_E_STATE.  After a full pass both entry points are valid.  After
 * dtsim_render_masked only dtsim_depth_masked is, and it must be given the mask the pass was given: on the quad-record pipelines both the
 * camera and the triangle set-up of the pass skip the unselected envs, whose records describe an older state (the generic pipelines write
 * every env's; the rule does not depend on the pipeline).  The masked call writes the rows of the selected envs only; the other rows keep
 * every byte.  One state gives the same bytes on every call, for every env index and whatever the other envs hold.
 * A null handle, out or mask, a non-positive or non-dividing size or an unknown flag return DTSIM_E_INVALID; a failed call launches
 * nothing and writes nothing.  Asynchronous, stream-ordered.
 * PER-ENV TABLES.  DTSIM_MAP_ENV_TABLES, accepted by dtsim_depth, dtsim_labels, dtsim_instances and their masked forms: read each env's own
 * distortion table if per-env tables are installed (dtsim_set_distortion_luts).  Let p = (i sy + sy / 2) cam_width + (j sx + sx / 2) and
 * s = src_index[env_cal[e]][p].  out[e][i][j] is then the value this pass gives at RECTILINEAR camera pixel s of env e -- the source pixel is
 * s itself, with its four MSAA samples, and every rule above applies unchanged -- and 0 where s = -1 (as in the black border).  That is the
 * surface whose colour the render pass's gather put at frames[e][p].  Every other rule of STATE holds as it stands.  Without installed tables
 * the flag changes nothing: the same kernel, the same bytes.  Without the flag, installed tables are refused as before.
 * Out of scope under per-env tables: the line and LED overlays (still refused), and folding the tables into the raster. */
enum { DTSIM_DEPTH_F16 = 1u };
#define DTSIM_MAP_ENV_TABLES 0x100u
int dtsim_depth(dtsim_t* h, void* out, int oh, int ow, uint32_t flags);
int dtsim_depth_masked(dtsim_t* h, void* out, int oh, int ow, uint32_t flags, const uint8_t* mask);
/* The semantic label map of every camera frame, on the device: WHICH surface a pixel shows, as a class id beside the observation and the
 * depth map (the reference has only the segment view: a colour picture with blended edges, in place of the frame).
 * THE QUANTITY.  labels[e][i][j], a uint8, is the class of the surface that sets depth[e][i][j] of dtsim_depth: of the four MSAA samples
 * of the frame's source pixel, the sample with the smallest eye depth.
 *   - Ties go to the lowest sample index.
 *   - A sky sample counts as +inf: it wins only if all four are sky.
 *   - Within a sample a mesh owns it only where its z-buffer depth is strictly smaller than the plane's (the colour pass's depth test).
 * The owner of that sample maps to the class:
 *   - a pixel the distortion table leaves without a source    DTSIM_LABEL_NONE
 *   - the clear colour                                         DTSIM_LABEL_SKY
 *   - the ground quad                                          DTSIM_LABEL_GROUND
 *   - a tile              texel_class[tex][v][u], the class of the NEAREST texel of the tile's texture at the hit: the texel coordinates are
 *                         those the generic raster filters at (from the tile's angle and the hit's wx, wz), rounded down after the
 *                         half-texel shift is taken back, wrapped as GL_REPEAT; a present tile without a texture: DTSIM_LABEL_GROUND
 *   - mesh object o       mesh_class[mesh id of o]
 * The device applies no colour rule and knows no class beyond these three: every other id is what the tables of
 * dtsim_set_label_assets say.  Ids 3 .. 7 are reserved for the default tile classes of the host (dtsim/labels.py), 8 .. 255 for objects.
 * Never filtered, never blended: an edge pixel carries the class of its nearest sample, not a mixture.
 * SIZE.  out: DEVICE pointer to [num_envs][oh][ow] bytes; size and sampling are dtsim_depth's: cam_height % oh == 0 and cam_width % ow == 0,
 * out[e][i][j] belongs to camera pixel (i sy + sy / 2, j sx + sx / 2), and only those pixels are traced.  flags: 0 or DTSIM_MAP_ENV_TABLES
 * (dtsim_depth's PER-ENV TABLES: the class at rectilinear pixel s of the env's own table, DTSIM_LABEL_NONE where s = -1).
 * TABLES.  dtsim_set_label_assets: texel_class[t] is [height][width] bytes in the row order and size of texture t of dtsim_set_assets,
 * mesh_class is [n_meshes]; both counts must mirror dtsim_set_assets (else DTSIM_E_INVALID), host pointers, copied during the call.  A
 * failed call changes nothing; dtsim_set_assets drops the tables (the list they mirror is gone).
 * STATE.  The rules of dtsim_depth, word for word (a colour render of the current state, the same calls invalidate, after
 * dtsim_render_masked only the masked form with the pass's mask, per-env distortion tables refused without DTSIM_MAP_ENV_TABLES), and
 * DTSIM_E_STATE without label tables.  A null handle, out or mask, a bad size or an unknown flag return DTSIM_E_INVALID; a failed call launches nothing and writes
 * nothing.  Asynchronous, stream-ordered.  One state gives the same bytes on every call and for every env index. */
enum { DTSIM_LABEL_NONE = 0, DTSIM_LABEL_SKY = 1, DTSIM_LABEL_GROUND = 2,
       DTSIM_LABEL_FLOOR = 3,        /* a non-drivable tile */
       DTSIM_LABEL_ROAD = 4, DTSIM_LABEL_MARK_WHITE = 5, DTSIM_LABEL_MARK_YELLOW = 6, DTSIM_LABEL_MARK_RED = 7,
       DTSIM_LABEL_OBJECT_FIRST = 8 };
int dtsim_set_label_assets(dtsim_t* h, const uint8_t* const* texel_class, int n_textures, const uint8_t* mesh_class, int n_meshes);
int dtsim_labels(dtsim_t* h, uint8_t* out, int oh, int ow, uint32_t flags);
int dtsim_labels_masked(dtsim_t* h, uint8_t* out, int oh, int ow, uint32_t flags, const uint8_t* mask);
/* The instance map of every camera frame, on the device: WHICH OBJECT a pixel shows, beside the class the label map gives -- the ground
 * truth of detection (the label map says "duckie", not which one; connected components of it merge duckies that touch or occlude each other).
 * THE QUANTITY.  inst[e][i][j], a uint8, names the owner of the sample that sets depth[e][i][j] of dtsim_depth: of the four MSAA samples of
 * the frame's source pixel, the sample with the smallest eye depth.
 *   - Ties go to the lowest sample index.
 *   - A sky sample counts as +inf: it wins only if all four are sky.
 *   - Within a sample a mesh owns it only where its z-buffer depth is strictly smaller than the plane's (the colour pass's depth test).
 * The value is o + 1 where that owner is mesh object o, and DTSIM_INSTANCE_NONE = 0 everywhere else: tile, ground quad, sky, or a pixel the
 * distortion table leaves without a source.  o is the object's index in the object list of the env's OWN map (dtsim_map.objects in the
 * order given to dtsim_set_maps): the column of the DTSIM_FIELD_OBJ_* fields, 0 .. DTSIM_MAX_OBJECTS - 1, so the id fits the byte.  An
 * invisible object (DTSIM_FIELD_OBJ_VISIBLE = 0) has no triangles in the pass: its id never appears.  Never filtered, never blended.
 * LABELS.  `labels` may be NULL.  If it is not, it receives exactly the bytes dtsim_labels writes for the same size -- from the same
 * classification of every pixel, in the same launch -- and the call needs the label tables (else DTSIM_E_STATE); where inst is o + 1 the
 * label is mesh_class[mesh id of o], where inst is 0 it is a plane's or a texel's class.  inst and labels must not overlap.
 * SIZE, STATE.  dtsim_depth's, word for word: [num_envs][oh][ow] bytes, cam_height % oh == 0 and cam_width % ow == 0, point-sampled at
 * camera pixel (i sy + sy / 2, j sx + sx / 2); a colour render of the current state must precede, the same calls invalidate, after
 * dtsim_render_masked only the masked form with the pass's mask (it writes the selected envs' rows only), per-env distortion tables are
 * refused without DTSIM_MAP_ENV_TABLES.  flags: 0 or DTSIM_MAP_ENV_TABLES (dtsim_depth's PER-ENV TABLES: the owner at rectilinear pixel s of
 * the env's own table, DTSIM_INSTANCE_NONE where s = -1; `labels` likewise).  A null handle, inst or mask, a bad size or an unknown flag
 * return DTSIM_E_INVALID; a failed call launches
 * nothing and writes nothing.  Asynchronous, stream-ordered.  One state gives the same bytes on every call and for every env index. */
enum { DTSIM_INSTANCE_NONE = 0 };
int dtsim_instances(dtsim_t* h, uint8_t* inst, uint8_t* labels, int oh, int ow, uint32_t flags);
int dtsim_instances_masked(dtsim_t* h, uint8_t* inst, uint8_t* labels, int oh, int ow, uint32_t flags, const uint8_t* mask);
/* One 2-D box and one visible-pixel count per id and env of an id map, on the device: the reduction of dtsim_instances' map to detection
 * targets.  Pure and stateless: not a post-pass of a render, it reads nothing but `inst`, any [num_envs][oh][ow] uint8 DEVICE map with
 * oh, ow >= 1 and oh * ow <= INT32_MAX (the size is not tied to the camera's).
 *   out: DEVICE pointer to [num_envs][DTSIM_MAX_OBJECTS][5] int32.  Row k describes id k + 1: x0, y0, x1, y1, n -- n the number of map
 *        pixels with that id, [x0, x1) x [y0, y1) their tight bound in map pixel coordinates (column, row); all five 0 when n == 0.
 *        Id 0 and ids above DTSIM_MAX_OBJECTS are ignored.  The boxes are in the map's own resolution.
 *   mask: DEVICE pointer to num_envs bytes, or NULL = every env; as dtsim_obs_push: the rows of unselected envs keep every byte.
 * Integer min / max / sums within one workgroup per env: one map gives one result, bit for bit.  16-byte loads over the part of an env's
 * bytes that lies between 16-byte boundaries, whatever the base's alignment.  A null handle, inst or out, a non-positive size, a product
 * beyond int32 or nonzero flags return DTSIM_E_INVALID, and nothing is launched.  Asynchronous, stream-ordered. */
int dtsim_boxes(dtsim_t* h, const uint8_t* inst, int oh, int ow, int32_t* out, uint32_t flags, const uint8_t* mask);
/* The egocentric bird's-eye label map of every env, on the device: WHAT LIES ON THE FLOOR around the robot, in metres and in the robot's own
 * frame -- the target of camera-to-BEV heads, the input of a privileged critic or planner.  It is the one per-cell output that does not
 * depend on the camera: defined under per-env distortion tables, under any fisheye, with or without a render pass.  The reference has no
 * such output (its nearest relatives: the top_down render mode); a learner-side addition like depth, labels and instances.
 * THE QUANTITY.  The call gives (oh, ow), cell (metres per cell, finite, > 0) and rows_behind (0 .. oh).  Env e has the AGENT's pose
 * (x, z, theta) = (cur_pos.x, cur_pos.z, cur_angle) -- DTSIM_FIELD_POS / DTSIM_FIELD_ANGLE, not the camera's --, forward d = (cos theta,
 * -sin theta) and right r = (sin theta, cos theta), both in (x, z), as get_dir_vec / get_right_vec.  Cell (i, j), row 0 the farthest ahead
 * and column 0 the leftmost, stands for the world point
 *     P = (x, z) + f d + s r,   f = (oh - rows_behind - i - 0.5) cell,   s = (j + 0.5 - ow / 2) cell      (ow / 2 is not rounded)
 * and the map is point-sampled at P, never filtered.  cls[e][i][j], a uint8, is the first of these that applies:
 *   1. a visible object's footprint: the lowest object index o of the env's own map with DTSIM_FIELD_OBJ_VISIBLE set and a mesh
 *      (mesh_id >= 0) whose collision rectangle contains P -- for a static object the four corners the host packed (dtsim_object.corners),
 *      for a dynamic one (duckies, followers, the checkerboard) the env's current corners, the rectangle _collision tests and draw_bbox
 *      draws, as stale as the physics leaves its axes.  The class is mesh_class[mesh id of o] of dtsim_set_label_assets.
 *   2. a present, textured tile that P lies on: the class of the NEAREST texel of its texture, by dtsim_labels' own statement (the texel
 *      coordinates the generic raster filters at, rounded down after the half-texel shift is taken back, wrapped as GL_REPEAT, the same
 *      texel_class pool): a camera label pixel and a cell that hit one world point name one class.
 *   3. anything else -- an untextured or absent tile, any point off the grid: DTSIM_LABEL_GROUND.
 * DTSIM_LABEL_NONE and DTSIM_LABEL_SKY never occur.  inst[e][i][j], from the same classification in the same launch, is o + 1 in case 1 and
 * DTSIM_INSTANCE_NONE otherwise: the ids of dtsim_instances.  Not drawn: the agent's own rectangle (the same cells in every env), heights,
 * occlusion (the view sees through everything).  The pose is read in float64 and the sine and cosine are taken of the float64 angle
 * (cur_angle is unbounded); a cell's P is then float32 arithmetic, within 1e-5 m of the float64 value while coordinates stay below 32 m.
 * SIZE.  cls, inst: DEVICE pointers to [num_envs][oh][ow] bytes each; either may be NULL, not both, and they must not be one buffer.
 * 1 <= oh, ow <= DTSIM_BEV_MAX_SIDE.  mask: DEVICE pointer to num_envs bytes, or NULL = every env; the rows of unselected envs keep every byte.
 * STATE.  Not a post-pass: it reads the pose, map id, object visibility and dynamic corners of the CURRENT state and the scene tables, so no
 * dtsim_render need precede it; the handle must hold the render tables (DTSIM_F_RENDER, dtsim_set_assets, dtsim_set_maps) and, with cls,
 * the label tables.  DTSIM_E_INVALID, before anything is launched or written, for: a null handle, both maps null or one buffer, a handle
 * without render tables, cls without label tables, a size outside 1 .. DTSIM_BEV_MAX_SIDE, a non-finite or non-positive cell, rows_behind
 * outside 0 .. oh, nonzero flags.  Asynchronous, stream-ordered, no host synchronisation.  One state gives the same bytes on every call,
 * for every env index and whichever of the two maps are asked for. */
#define DTSIM_BEV_MAX_SIDE 1024
int dtsim_bev(dtsim_t* h, uint8_t* cls, uint8_t* inst, int oh, int ow, double cell, int rows_behind, uint32_t flags, const uint8_t* mask);
/* The ground-projected camera image of every env, on the device: Duckietown's ground projection (inverse perspective mapping), the CAMERA
 * FRAME WARPED ONTO THE FLOOR PLANE in the robot's own frame -- the input a camera-to-BEV head is compared against, in dtsim_bev's cell
 * geometry: cell (i, j) here and cell (i, j) of dtsim_bev with the same (oh, ow), cell and rows_behind name one world point.  A learner-side
 * addition; the reference has no such output.
 * THE QUANTITY.  (oh, ow), cell and rows_behind mean what they mean in dtsim_bev and have its limits.  Cell (i, j) of env e stands for the
 * point P = (x, z) + f d + s r on the TILE PLANE y = 0, with dtsim_bev's f, s, d, r of the agent's pose.  Everything below is float64.
 *   1. The camera (oracle/raster.py Camera).  Centre C = pos [+ the camera noise of DTSIM_FIELD_CAMERA, in world axes, where the handle
 *      renders per-env cameras: DTSIM_F_DOMAIN_RAND] + (0.066 cos theta, cam_height, -0.066 sin theta); pitch and fov_y the env's own
 *      float32 values of DTSIM_FIELD_CAMERA promoted to double, or on the shared camera 0.108 m, 19.15 and 75 degrees; ty = tan(fov_y / 2),
 *      tx = ty W / H.  Eye coordinates as Camera.to_eye; w = -z_eye; u = (x_eye / w / tx + 1) W / 2, v = (1 - y_eye / w / ty) H / 2 -- pixel c
 *      spans [c, c + 1): the projection of dtsim_draw_lines.
 *   2. Rectilinear frames (no calibration installed): the source pixel is (r, c) = (floor v, floor u).
 *   3. Fisheye frames (dtsim_set_ipm_calibrations): the calibration's forward model -- cv::initUndistortRectifyMap's arithmetic with the
 *      env's own K, D and new_K at the real-valued index coordinates (u - 0.5, v - 0.5) -- gives the distorted coordinates (xd, yd), and
 *      (r, c) = (floor(yd + 0.5), floor(xd + 0.5)).  No table is read, so a calibration per env is defined too.  A PROPERTY OF THE
 *      REFERENCE'S FISHEYE, not a tolerance: its frames are made with an approximate INVERSE table (_invert_map, _fill_holes), so the
 *      rectilinear pixel that frame pixel (r, c) actually shows lies a median 0.8 px from the aimed (u, v), p99 2.1 px, at most 4.2 px
 *      (640 x 480, four map shapes, measured on the host).
 *   4. The cell is valid iff w >= 0.04 (the near plane), with a fisheye (u, v) lies inside [0, W) x [0, H), and (r, c) lies inside the frame.
 *   5. img[e][i][j][0..2] -- [e][0..2][i][j] with DTSIM_IPM_CHW -- are the three bytes at (r, c) of env e's frame in the handle's current
 *      frame batch (dtsim_bind_frames' buffer or the internal one, as dtsim_observe reads it), 0, 0, 0 where the cell is invalid;
 *      valid[e][i][j] is 1 or 0; src[e][i][j] is r W + c, or -1: with it any camera map of the frame's size (depth, labels, instances) is
 *      ground-projected by one gather.
 * Sampling is nearest-pixel, never filtered.  It is a FLAT-WORLD projection: no occlusion, and whatever stands on the floor smears away
 * from the camera.  The frames are read as they are: no dtsim_render need precede the call, and it does not know which state they show.
 * SIZE.  img: DEVICE pointer to num_envs * oh * ow * 3 bytes, valid: to num_envs * oh * ow bytes, src: to as many int32.  Any subset, not
 * none, no two one buffer.  mask: DEVICE pointer to num_envs bytes, or NULL = every env; the rows of unselected envs keep every byte.
 * DTSIM_E_INVALID, before anything is launched or written, for: a null handle, every output null or two of them one buffer, flags other
 * than DTSIM_IPM_CHW, a size outside 1 .. DTSIM_BEV_MAX_SIDE, a non-finite or non-positive cell, rows_behind outside 0 .. oh.  DTSIM_E_STATE
 * before the first dtsim_reset or on a handle without DTSIM_F_RENDER.  Asynchronous, stream-ordered, no host synchronisation.  One state
 * and one frame batch give the same bytes on every call, for every env index and whichever outputs are asked for.
 * With the shared camera and at most one calibration the cell -> pixel map is the same for every env and step: the handle computes it
 * once per (oh, ow, cell, rows_behind, calibration) into a table of its own and the call is one gather (the first such call of a handle
 * allocates the table, 4 MB, which is the one device allocation the entry point ever makes).
 *
 * dtsim_set_ipm_calibrations: the calibrations of step 3.  K, new_K: [n_cal][3][3], D: [n_cal][5] (k1, k2, p1, p2, k3), env_cal: [num_envs]
 * indices in [0, n_cal) -- all HOST pointers, copied.  new_K is the caller's (the reference computes it for 640 x 480 at any camera
 * size); it must have an inverse.  env_cal may be NULL when n_cal = 1.  n_cal = 0 (every pointer NULL): rectilinear, a new handle's state.
 * DTSIM_E_INVALID for a null handle, n_cal < 0, a missing table, a value that is not finite, an index out of range; DTSIM_E_STATE without
 * DTSIM_F_RENDER.  A failed call changes nothing.  Synchronises the stream. */
#define DTSIM_IPM_CHW 1u
int dtsim_set_ipm_calibrations(dtsim_t* h, int n_cal, const double* K, const double* D, const double* new_K, const int32_t* env_cal);
int dtsim_ipm(dtsim_t* h, uint8_t* img, uint8_t* valid, int32_t* src, int oh, int ow, double cell, int rows_behind, uint32_t flags,
              const uint8_t* mask);
/* The optical-flow map of every camera frame, on the device: HOW THE PICTURE MOVED since a remembered state -- the ground truth of
 * optical-flow and ego-motion heads and of warping losses, beside the maps above, which all describe one state.  A learner-side addition;
 * the reference has no such output.
 * THE QUANTITY.  For output pixel (i, j) of env e, camera pixel p is chosen by dtsim_depth's SIZE rule and its source pixel by dtsim_depth's
 * rule.  Let q be the sample that sets dtsim_depth's value there: the smallest eye depth of the four MSAA samples, ties to the lowest index,
 * sky counting as +inf; its owner is chosen as dtsim_labels chooses it (a mesh only where its z-buffer depth is strictly smaller than the
 * plane's).  X is the eye-space hit of q's ray at that depth, P the world point it stands for.
 *   - The previous point.  If the owner is a plane (tile, ground quad), P_prev = P.  If it is mesh object o, the point moves with the object:
 *     P_prev = pos_prev(o) + Ry(yrot_prev(o)) Ry(yrot_cur(o))^-1 (P - pos_cur(o)), pos and yrot being what the render pass places the mesh
 *     with -- a static object's own (the motion is the identity), a dynamic one's DTSIM_FIELD_OBJ_CENTER, its height + DTSIM_FIELD_OBJ_Y and
 *     DTSIM_FIELD_OBJ_YROT.  "Previous" is the state the last dtsim_flow_mark remembered for the env.
 *   - flow = A(proj_prev(P_prev)) - A(proj_cur(P)), in CAMERA pixels, x to the right and y down, whatever the map's size.  Previous minus
 *     current: prev_frame[p + flow] is what cur_frame[p] shows.  proj is dtsim_ipm's step 1 with each state's own camera (height, pitch,
 *     fov_y and noise of DTSIM_FIELD_CAMERA on per-env cameras, else the shared one), formed in float64 from the float64 poses: the camera
 *     centres are subtracted before anything is rounded to the float32 record a pixel applies.  A is the identity on rectilinear frames; on
 *     fisheye frames it is the forward model of dtsim_ipm's step 3 at (u - 0.5, v - 0.5), with calibration 0 of dtsim_set_ipm_calibrations.
 *     Both terms go through the same functions.  As in dtsim_ipm, A PROPERTY OF THE REFERENCE'S FISHEYE, not a tolerance: the frame itself
 *     is made with an approximate INVERSE table, so what frame pixel p shows lies a median 0.8 px (at most 4.2 px at 640 x 480) from A's value.
 *   - valid[e][i][j] is 1 iff the pixel has a source pixel, q is not sky, the env has a mark of its current episode (DTSIM_FIELD_EPISODE
 *     and DTSIM_FIELD_MAP_ID at the mark equal the current values), w_prev >= 0.04 and the previous rectilinear (u, v) lies in
 *     [0, W) x [0, H).  An invalid pixel has flow 0, 0.
 *   - Where nothing moved between the mark and the call (the same pose, the same camera, an object with the same pose) the flow is
 *     exactly 0.0: every rotation enters the record as the rotation by a float64 angle DIFFERENCE, never as a product that ought to cancel.
 * Out of scope: sky pixels, forward flow, occlusion masks, half precision, per-env distortion tables (refused, DTSIM_MAP_ENV_TABLES
 * included), frames that show UndistortWrapper's view.
 * dtsim_flow_mark remembers, for the selected envs (mask: DEVICE pointer to num_envs bytes, or NULL = every env), what the flow needs of the
 * CURRENT state: the float64 pose, the six camera floats, episode and map id, and per dynamic slot centre, height and y_rot.  It reads the
 * state arrays, not what a render left: it needs no render and is valid after a masked pass.  The marks live in a buffer of the handle,
 * outside the state blob (DTSIM_FIELD_STATE_BLOB does not carry them); dtsim_set_maps and dtsim_set_assets drop all marks.  DTSIM_E_STATE
 * before the first dtsim_reset.  Asynchronous, stream-ordered.
 * SIZE.  flow: DEVICE pointer to [num_envs][2][oh][ow] float32 (plane 0: x, plane 1: y); valid: to [num_envs][oh][ow] bytes, or NULL.
 * cam_height % oh == 0 and cam_width % ow == 0; the map is dtsim_depth's point sample, full[:, :, sy/2::sy, sx/2::sx].  flags must be 0.
 * STATE.  dtsim_depth's rules, word for word: a colour dtsim_render of the CURRENT state must precede, the same calls invalidate, after
 * dtsim_render_masked only dtsim_flow_masked with the pass's mask is valid (it writes the selected envs' rows only), installed per-env
 * distortion tables are refused; and a handle whose distortion table is a fisheye's needs dtsim_set_ipm_calibrations first.  All
 * DTSIM_E_STATE.  A null handle, flow or mask, flow and valid one buffer, a bad size or nonzero flags return DTSIM_E_INVALID.  A failed call
 * launches nothing and writes nothing.  Asynchronous, stream-ordered.  One state and one mark give the same bytes on every call and for
 * every env index. */
int dtsim_flow_mark(dtsim_t* h, const uint8_t* mask);
int dtsim_flow(dtsim_t* h, float* flow, uint8_t* valid, int oh, int ow, uint32_t flags);
int dtsim_flow_masked(dtsim_t* h, float* flow, uint8_t* valid, int oh, int ow, uint32_t flags, const uint8_t* mask);

/* Depth, labels, instances and flow of ONE size from one launch: the learner that turns several of them on pays the classification of a pixel
 * -- four samples against the planes and the z-buffer of the env's projected triangles, which is the cost of each single pass -- once.
 * THE QUANTITY, by reference.  Every non-null output is the quantity of its own entry point -- depth: dtsim_depth's (half with
 * DTSIM_DEPTH_F16), labels: dtsim_labels', instances: dtsim_instances', flow / flow_valid: dtsim_flow's -- and all come from ONE classification
 * of the pixel: the sample with the smallest eye depth, ties to the lowest index, sky counting as +inf.  So where instances is o + 1, labels is
 * the class of object o's mesh; depth is the depth of the sample that owns labels and instances; flow is the motion of that sample's surface
 * point.  The triangles are tested as every single pass tests them (the boxes of the render pass itself: a triangle it culled is skipped).
 * SIZE.  dtsim_depth's, one (oh, ow) for all outputs; the shapes are those of the single entry points.  flags: DTSIM_DEPTH_F16 and
 * DTSIM_MAP_ENV_TABLES (dtsim_depth's PER-ENV TABLES), nothing else.
 * STATE.  dtsim_depth's rules; labels needs dtsim_set_label_assets; with flow also dtsim_flow's rules: a fisheye handle needs
 * dtsim_set_ipm_calibrations, installed per-env distortion tables are refused with or without DTSIM_MAP_ENV_TABLES, and -- where dtsim_flow
 * answers with an all-zero map -- a handle on which dtsim_flow_mark has never been called is refused (an env without a mark of its episode
 * still gets flow 0, valid 0).  All DTSIM_E_STATE.  DTSIM_E_INVALID: a null handle, struct or mask, all five pointers null, flow_valid without
 * flow, outputs that overlap, a bad size, an unknown flag.  A failed call launches nothing and writes nothing.  With flow the call first
 * brings the envs' flow records up to date, as dtsim_flow does.  Asynchronous, stream-ordered.  One state (and one mark) gives the same bytes
 * on every call and for every env index.  The masked form: as dtsim_depth_masked, for every output. */
typedef struct dtsim_camera_maps_out {
  void* depth;            /* [N][oh][ow] float32, or half with DTSIM_DEPTH_F16; or NULL */
  uint8_t* labels;        /* [N][oh][ow]; or NULL (needs the label tables, else DTSIM_E_STATE) */
  uint8_t* instances;     /* [N][oh][ow]; or NULL */
  float* flow;            /* [N][2][oh][ow]; or NULL (needs marks as dtsim_flow does) */
  uint8_t* flow_valid;    /* [N][oh][ow]; or NULL; needs flow */
} dtsim_camera_maps_out;
int dtsim_camera_maps(dtsim_t* h, const dtsim_camera_maps_out* out, int oh, int ow, uint32_t flags);
int dtsim_camera_maps_masked(dtsim_t* h, const dtsim_camera_maps_out* out, int oh, int ow, uint32_t flags, const uint8_t* mask);

/* Geometry queries of the reference at arbitrary poses, evaluated on the device against
 * env env_idx[q]'s world (its map, dynamic objects and visibility): _valid_pose,
 * _collision, _drivable_pos, get_lane_pos2, closest_curve_point, proximity_penalty2,
 * compute_reward, _inconvenient_spawn.  poses: [n][3] = x, z, angle.  Synchronous. */
int dtsim_query(dtsim_t* h, int n, const int32_t* env_idx, const double* poses,
                double safety_factor, dtsim_probe* out);

/* Everything Simulator.step hands back about ONE env besides the observation -- cur_pos / cur_angle / speed /
 * timestamp (simulator.py:1551-1584), _compute_done_reward (:1685-1705), get_agent_info (:1586-1612) -- gathered
 * on the device and copied with one transfer (a 1-env gym loop otherwise pays one dtsim_read per value).
 * Synchronous. */
typedef struct dtsim_agent_info {
  double pos[3], angle, speed, timestamp;
  double wheels[2];         /* last [left, right] duty passed to the dynamics */
  double lane[4];           /* dist, dot_dir, angle_deg, angle_rad (0 if not in lane) */
  double prox, reward;
  int32_t tile[2], step_count;
  uint8_t in_lane, done, done_code, pad;
} dtsim_agent_info;
int dtsim_read_agent(dtsim_t* h, int env, dtsim_agent_info* out);

int dtsim_read(dtsim_t* h, int field, void* dst, size_t bytes);   /* synchronous D2H */
int dtsim_write(dtsim_t* h, int field, const void* src, size_t bytes);
void* dtsim_field_devptr(dtsim_t* h, int field);
size_t dtsim_field_bytes(const dtsim_t* h, int field);
size_t dtsim_state_bytes(const dtsim_t* h);

int dtsim_sync(dtsim_t* h);
void* dtsim_stream(dtsim_t* h);   /* the hipStream_t launches go to */
/* Sum of HIP-event durations of the launches of `kernel` since the last call
 * (requires DTSIM_F_PROFILE).  Synchronises the stream. */
int dtsim_profile_read(dtsim_t* h, int kernel, int* n_launches, double* total_ms);

#ifdef __cplusplus
}
#endif
#endif /* DTSIM_H */
