/*
 * ffmp.h — C ABI of libffmp, the MI355X (gfx950) batched flow-field
 * motion-planning environment (the `gym_ffmp` step/reset hot path).
 *
 * Every buffer is caller-owned, contiguous, env-major DEVICE memory (in
 * practice torch tensors' data_ptr()).  Nothing here allocates (except the
 * optional frame-ring helper ffmp_ring_create at the end), prints or throws.
 * Each call enqueues work on `stream` (a hipStream_t passed as void*;
 * NULL = the legacy default stream) and returns 0, or a negative FFMP_E_* code
 * with a message readable from ffmp_last_error() (thread-local).
 *
 * Reference interfaces each entry point replaces (paths relative to the
 * reference repo YoshitakaNagai/flow_field_based_motion_planner):
 *   ffmp_reset          -> the external /episode_manager + is_first branch of
 *                          src/train.py:532-566 (start/goal, temporal stack
 *                          duplication, velocity := 0, d0 := dist) and the
 *                          commented-out FFMP.reset src/gym_ffmp/envs/ffmp.py:77-83
 *   ffmp_set_scenario   -> the same is_first branch with the episode /episode_manager
 *                          publishes on /start_goal_points (src/train.py:86,88,113-132)
 *                          given by the caller instead of sampled
 *   ffmp_step, ffmp_step_fused -> one iteration of src/train.py:523-693 with Gazebo
 *                          (/cmd_vel integration), /bev_* rasterisers and
 *                          rewarder2 (src/gym_ffmp/envs/ffmp.py:179-188) in-GPU
 *   ffmp_step_state_cmd, ffmp_step_fused_cmd, ffmp_step_cmd -> the same iteration driven by a
 *                          continuous (v, w) command: the action Box of
 *                          src/gym_ffmp/envs/ffmp.py:29-32 published as a Twist by
 *                          cmd_vel_publisher (src/train.py:134-143)
 *   ffmp_ring_*, ffmp_dlpack -> storage of make_temporal_maps' 2-frame stack
 *                          (src/train.py:474-486) kept in place (optional helper)
 *   ffmp_temporal_maps  -> make_temporal_maps over INPUT_CHANNELS = k mono frames
 *                          (src/train.py:66-69, 474-486) served from the frame ring
 *   ffmp_bev_image      -> the (occupancy + flow(RGB)) image of the 12-channel option
 *                          (src/train.py:66, src/gym_ffmp/envs/ffmp.py:16)
 *   ffmp_raster         -> external /bev_flow_estimator + /temporal_bev_publisher
 *                          (src/train.py:116-121, make_temporal_maps :474-486)
 *   ffmp_visible_frames -> what the sensor-driven /bev_flow_estimator can show of those frames
 *                          (/bev/temporal_bev_image, src/train.py:116-121): nothing an obstacle
 *                          hides from the robot; the node is outside the reference's repository,
 *                          so the line-of-sight rule is this header's own [unpinned]
 *   ffmp_scan_frames    -> the same image built from the robot's own /scan (the L ranges of the
 *                          LaserScan, src/train.py:87,145-150) instead of from ground truth: an
 *                          inverse sensor model, this header's own [unpinned]
 *   ffmp_scan_map       -> that image with a memory: int8 log-odds per cell, moved with the
 *                          robot's own motion and updated from every scan [unpinned]
 *   ffmp_world_map / ffmp_world_frame -> the /map a ROS graph keeps beside /scan and /odom: int8
 *                          log-odds per WORLD cell, never re-sampled, and its ego view [unpinned]
 *   ffmp_scan_match     -> the pose corrected against that /map before the scan is integrated: a
 *                          correlative search over cell shifts and rotation steps [unpinned]
 *   ffmp_scan_relocalize -> the same winner over the whole plane and the full circle, with no prior:
 *                          a pruned two-level correlative search [unpinned]
 *   ffmp_scan_flow      -> the flow half of that image (the RGB of "occupancy(MONO) + flow(RGB)",
 *                          src/gym_ffmp/envs/ffmp.py:16) from two scan frames and the two poses: a
 *                          per-cell velocity by block matching with ego-motion compensation [unpinned]
 *   ffmp_flow_predict   -> what the planner makes of that flow: the frame with the cells a moving
 *                          obstacle will cover when the robot can be there marked occupied [unpinned]
 *   ffmp_frame_potential -> the potential plane and its gradient (obs.potential, obs.grad) from any of
 *                          those frames instead of from the simulator's discs, and the clearance
 *                          plane underneath [unpinned]
 *   ffmp_dwa            -> a dynamic-window / trajectory-rollout planner over that cost-to-go plane and
 *                          that flow: the reference's 28 commands (config.py:28-55) rolled forward,
 *                          rejected where they meet an obstacle at the time the robot is there [unpinned]
 *   ffmp_reward_done    -> FFMP.rewarder / rewarder2 / reward_calculator /
 *                          is_goal / is_done (src/gym_ffmp/envs/ffmp.py:120-188)
 *   ffmp_footprint_collision -> FFMP.is_collision (ffmp.py:85-105)
 *   ffmp_scan_collision[_f64] -> FFMP.is_collision2 (ffmp.py:108-117)
 *   ffmp_footprint      -> the robot_grids mask built inside is_collision
 *                          (ffmp.py:87-94), host-side, float64
 *   ffmp_episode_init / ffmp_episode_update -> the main loop's episode
 *                          bookkeeping: counters src/train.py:501-505, reach_times /
 *                          reach_rate :579-587 (REACH_MEMORY_CAPACITY :76), is_first
 *                          :593,662, truncation :607, the is_done branch :611-682
 *                          (episode / step / total_step, completion test :644)
 */
#ifndef FFMP_H
#define FFMP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FFMP_ABI_VERSION 9  /* 9: ffmp_step_state_cmd, ffmp_step_fused_cmd, ffmp_step_cmd, ffmp_policy_field */
#define FFMP_MAX_OBST 64     /* K  */
#define FFMP_MAX_FOOT 128    /* footprint cells */
#define FFMP_MAX_BEAMS 1024  /* L  */
#define FFMP_N_ACTIONS 28
#define FFMP_REC_HDR 16      /* floats of per-env raster-record header */

/* error codes */
#define FFMP_OK 0
#define FFMP_E_ARG (-1)
#define FFMP_E_HIP (-2)
#define FFMP_E_CFG (-3)

/* collide_mode bits */
#define FFMP_COLLIDE_FOOTPRINT 1
#define FFMP_COLLIDE_LIDAR 2

/* Configuration, passed by pointer and copied by value into each launch.
 * float64 fields drive the per-env scalar maths (as the reference's Python
 * floats do); the *_f fields are the float32 constants of the per-cell raster
 * and MUST equal (float)(the double expression) documented beside them — the
 * Python host (flow_field_based_motion_planner_amd/config.py) fills both. */
typedef struct ffmp_cfg {
  int32_t grid;          /* G: local map is G x G cells, G % 4 == 0, 8 <= G <= 4096 */
  int32_t n_obst;        /* K: obstacles per env, 0..FFMP_MAX_OBST */
  int32_t n_beams;       /* L: lidar beams, 0..FFMP_MAX_BEAMS (0 = no lidar) */
  int32_t max_steps;     /* truncation: done when t == max_steps (train.py:60,607) */
  int32_t moving;        /* 1: obstacles move and reflect off the world walls */
  int32_t autoreset;     /* 1: ffmp_step resets done envs in place */
  int32_t collide_mode;  /* FFMP_COLLIDE_* bits */
  int32_t n_foot;        /* number of footprint offsets below */
  int32_t flow;          /* 1: raster the BEV motion-flow planes (obs.flow) */
  int32_t reserved0;
  int32_t foot_di[FFMP_MAX_FOOT]; /* footprint cell offsets from (G/2, G/2) */
  int32_t foot_dj[FFMP_MAX_FOOT];
  double res;            /* m per cell (ffmp.py:18, 0.05) */
  double dt;             /* s per step, >= 0 (0: nothing moves; the followers that divide by it refuse it) */
  double robot_r;        /* lidar collision threshold (ffmp.py:17, 0.13), >= 0 */
  double goal_thr;       /* goal threshold (ffmp.py:19, 0.5) */
  double world_half;     /* world is [-world_half, world_half]^2 (m) */
  double lidar_max;      /* lidar max range (m), >= 0; farther -> +inf */
  double goal_min, goal_max;   /* reset: goal distance range (m) */
  double obst_rmin, obst_rmax; /* reset: obstacle radius range (m) */
  double obst_vmax;            /* reset: obstacle speed range [0, vmax] (moving) */
  double start_clear, goal_clear; /* reset: clearance of obstacle surface from start / goal */
  /* float32 raster constants */
  float res_f;           /* (float)res */
  float half_f;          /* (float)(0.5 * (G * res)) : ego coordinate of cell 0 is -half_f */
  float world_half_f;    /* (float)world_half */
  float half_ka_f;       /* (float)(0.5 * k_att) */
  float half_kr_f;       /* (float)(0.5 * k_rep) */
  float rho0_f;          /* (float)rho0 : repulsive cut-off (m), > 0 */
  float inv_rho0_f;      /* (float)(1.0 / rho0) */
  float rho_min_f;       /* (float)rho_min : distance clamp (m) */
  float inv_2res_f;      /* (float)(1.0 / (2.0 * res)) : central-difference scale */
  float cull_margin_f;   /* (float)cull_margin : metres added to a disc's reach (and taken off the world's
                          * half side) by every cull, so that a float32 rounding never culls a disc or a
                          * wall a cell test would have seen.  Must be finite and at least
                          * 2^-16 S, S = G res / 2 + world_half + rho0 + obst_rmax: the culls' distances
                          * are bounded by S and differ from the cell tests' by fewer than 16 roundings
                          * of 2^-24 each (< 2^-20 S); the floor leaves a factor of 16 (3e-4 m at
                          * G = 256, res = 0.05; the default is 0.1).  Below it: FFMP_E_CFG.  A larger
                          * margin costs time only, never a bit of the planes. */
  uint64_t seed;         /* Philox4x32-10 key */
  const double* beam_cs; /* DEVICE (L,2) float64 {cos, sin} of beam angle -pi + l*2pi/L, 16-B aligned */
} ffmp_cfg_t;

/* Per-env simulator state (device pointers, N envs). */
typedef struct ffmp_state {
  double* pose;     /* (N,3) x, y, yaw                               */
  double* goal;     /* (N,2) world goal                              */
  double* d0;       /* (N)   pre_relative_goal_dist (ffmp.py:139)    */
  double* obst;     /* (N,K,4) x, y, vx, vy                          */
  double* obst_r;   /* (N,K) radius                                  */
  int32_t* t;       /* (N)   steps since episode start               */
  int32_t* episode; /* (N)   episode counter (RNG key part)          */
  float* record;    /* (N, FFMP_REC_HDR + 12K) raster record */
  uint32_t* err;    /* (1)   sticky error bits (value 1: bad action id, value 2: NaN command,
                       value 4: bad scenario, ffmp_set_scenario) */
  /* Optional (NULL = not written): the post-step state of every env BEFORE auto-reset, i.e. what
   * the reference loop observes on the iteration that ends an episode (train.py:543-557) —
   * consumers that store transitions (a replay memory) need it for done envs. Written by
   * ffmp_step / ffmp_step_state for all envs (equal to record / the small obs when not reset). */
  float* term_record; /* (N, FFMP_REC_HDR + 12K) */
  float* term_obs;    /* (N, 5) state_g[2], state_v[2], state_t */
} ffmp_state_t;

/* Observation plane formats (ffmp_obs_t.format).  F32: the reference consumer layout
 * (train.py:543-545 state_m float32 0/255; potential float32).  U8F16: a compact layout for
 * consumers that convert on load — state_m frames as uint8 0/255 (the same values) and the
 * potential plane as IEEE binary16 (float32 value rounded to nearest even); the state_m and
 * potential pointers then address uint8_t / binary16 elements and the state_m strides count
 * elements.  3 instead of 8 bytes per cell of a newest-only raster.  Flow planes (cfg.flow), when
 * present, are binary16 too (obs.flow then addresses binary16 elements). */
#define FFMP_OBS_F32 0
#define FFMP_OBS_U8F16 1

/* Observation tensors (device pointers).  Layout = reference train.py:44,543-557
 * with a leading N: state_m (N,2,G,G) [older, newest] values 0/255 as float. */
typedef struct ffmp_obs {
  float* state_m;   /* (N,2,G,G) */
  float* state_g;   /* (N,2) relative goal [dist, orient]          */
  float* state_v;   /* (N,2) per-step [|dxy|, wrap(dyaw)]          */
  float* state_t;   /* (N,1) dt (0 on the first step)              */
  float* potential; /* (N,G,G) attractive+repulsive potential, or NULL */
  float* grad;      /* (N,2) central-difference gradient at robot cell */
  float* lidar;     /* (N,L) ranges (+inf = no return, -inf = inside), NULL if L == 0 */
  float* flow;      /* (N,2,G,G) ego-frame velocity (m/s) of the disc covering each cell of the
                       newest frame (lowest disc index wins), 0 elsewhere; NULL unless cfg.flow */
  int64_t state_m_stride;       /* elements (floats) from env e's older frame to env e+1's; 0 = 2*G*G */
  int64_t state_m_frame_stride; /* floats from env e's older frame to its newest; 0 = G*G.
                                   0/0 is the contiguous (N,2,G,G) layout.  A slot-major frame
                                   window (W, N, G, G) uses G*G / N*G*G with state_m at the
                                   older slot (see FFMP_RASTER_NEWEST).  May be negative (the
                                   newest frame in a lower slot: a seamless ring's wrap step can
                                   write slot 0 through its first mapping instead of slot W's). */
  int32_t format;   /* FFMP_OBS_F32 (0) or FFMP_OBS_U8F16 */
  int32_t reserved; /* 0, or FFMP_OBS_EXT_* bits: what follows this struct in memory (below) */
} ffmp_obs_t;

/* Sparse frame stores (an addition within ABI 9: no existing symbol, struct size or value changes).
 * An occupancy frame is 0 outside the discs and the world's walls, and so is the frame the ring slot
 * held before, so almost every 16-byte frame store of a step writes 0.0f over 0.0f.  With granule
 * tags the raster skips those stores; every frame, plane and record word stays what the dense raster
 * writes.
 *   reserved == 0: today's behaviour, the ffmp_obs_t stands alone.
 *   reserved & FFMP_OBS_EXT_TAGS: the ffmp_obs_t* passed in points at the first member of an
 *   ffmp_obs_tags_t.  Read by every launch that rasters: ffmp_raster, ffmp_raster_ex, ffmp_step,
 *   ffmp_step_cmd, ffmp_step_fused, ffmp_step_fused_cmd, ffmp_step_skewed; ignored by the others.
 * A granule is 64 consecutive cells of a frame plane in linear order (cell q is in granule q / 64; the
 * last one of a plane may be partial), one tag byte per granule: T = ceil(G*G / 64) tags per frame.
 *   tags_older / tags_newest: the tags of the frames state_m[:, 0] / state_m[:, 1] address, env 0's
 *   first; env e's are tags_env_stride bytes further per env (>= T).  They belong to the MEMORY of a
 *   frame (a physical ring slot), not to the view: a slot mapped at two addresses (the seamless ring's
 *   slot 0) has one set of tags.  Device memory, no alignment.
 * Invariant: tag == 0  =>  all cells of that granule of that frame are 0.0f (+0).  tag == 1: unknown
 * or non-zero.  Any other value counts as 1.
 * Per frame it writes (the newest one; the older one too where it writes it), a launch stores a
 * granule's cells only if one of them is non-zero or the granule's tag is non-zero, and then sets the
 * tag to "one of them is non-zero".  Launch shapes whose store groups are not whole granules
 * (FFMP_RASTER_TILE8 / TILE16) and blocks of more than 65,536 cells store everything and write tag 1.
 * An env a launch skips (mask) keeps its cells and its tags.
 * Who may write a tagged frame: the launches above, through an ffmp_obs_tags_t that names the frame's
 * tags.  For every consumer the frames are read-only.  A caller that writes frame memory itself (a
 * memset, a copy, a launch without the flag, memory that is new or re-mapped) must set the tags of the
 * frames it touched to 1 before the next tagged launch; all-zero memory may take tags 0 instead.
 * FFMP_E_ARG (nothing launched): the flag with a NULL tag pointer, with tags_env_stride < T, or with
 * format != FFMP_OBS_F32 (the compact frames are stored densely). */
#define FFMP_OBS_EXT_TAGS 1
#define FFMP_TAG_CELLS 64
typedef struct ffmp_obs_tags {
  ffmp_obs_t obs;          /* obs.reserved & FFMP_OBS_EXT_TAGS */
  uint8_t* tags_older;     /* (N, T) tags of the frame at state_m */
  uint8_t* tags_newest;    /* (N, T) tags of the frame at state_m + state_m_frame_stride */
  int64_t tags_env_stride; /* bytes between consecutive envs' tags, >= T */
} ffmp_obs_tags_t;

/* Per-step outputs (device pointers, N each). Flags are 0/1 bytes. */
typedef struct ffmp_out {
  float* reward;
  uint8_t* done;
  uint8_t* is_goal;
  uint8_t* collide;
  uint8_t* truncated;
} ffmp_out_t;

int ffmp_abi_version(void);
const char* ffmp_last_error(void);

/* Layout check for FFI bindings: which = 0 sizeof(ffmp_cfg_t), 1 sizeof(ffmp_state_t),
 * 2 sizeof(ffmp_obs_t), 3 sizeof(ffmp_out_t), 4 offsetof(ffmp_cfg_t, res),
 * 5 offsetof(ffmp_cfg_t, res_f), 6 offsetof(ffmp_cfg_t, seed),
 * 7 offsetof(ffmp_cfg_t, beam_cs), 8 sizeof(ffmp_episode_t),
 * 9 offsetof(ffmp_obs_t, format); the extension structs from 20 on: 20 sizeof(ffmp_obs_tags_t),
 * 21 offsetof(ffmp_obs_tags_t, tags_older); -1 otherwise (10 .. 19 included). */
int64_t ffmp_layout(int32_t which);

/* Launch-shape tuning (process-wide; not thread-safe against concurrent launches).
 * Returns the previous value (>= 0) or FFMP_E_ARG.  Never changes results (FFMP_TUNE_CONV_MFMA: the
 * convolutions' fp32 summation order). */
#define FFMP_TUNE_RASTER_CPB 1  /* raster cells per block: multiple of 1024; 0 = default   */
#define FFMP_TUNE_RASTER_NT 2   /* raster stores: 0 by plane size, 1 plain, 2 nontemporal  */
#define FFMP_TUNE_RASTER_XCD 3  /* 1: XCD-aware block remap                                */
#define FFMP_TUNE_ENV_WAVES 4   /* waves per env_kernel block: 1 or 4                       */
#define FFMP_TUNE_ENV_LANES 5   /* lanes per env in env_kernel: 0 auto, 4, 8, 16, 32, 64 (a lane holds ceil(K / lanes) discs) */
#define FFMP_TUNE_RING_EXTRA 6  /* ffmp_ring_create / rebuild: fresh pieces allocated beyond the
                                   ones the ring needs (pairing candidates; they stay pooled):
                                   0 = default (need/2 + 4), v >= 1 = at most v - 1.  An HBM
                                   budget (FFMPVec hbm_budget) sets it around its ring creation. */
#define FFMP_TUNE_CONV_MFMA 7   /* MFMA shape of the convolution kernels that have both: 0 (default, each
                                   kernel's measured fastest: 32x32x16 for the forwards, the data gradient and
                                   the 32 -> 64 weight gradient, 16x16x32 for the other weight gradients and
                                   the small-image padded data gradients), 16
                                   (v_mfma_f32_16x16x32_bf16) or 32 (v_mfma_f32_32x32x16_bf16); the same
                                   products, fp32 sums in another order */
#define FFMP_TUNE_CONV_KYS 8    /* kernel rows per ring step of the row-ring convolution forward: 0 (default,
                                   1), 1, 2 or 4 (the same products and sums) */
#define FFMP_TUNE_CONV_LB 9     /* 1: the unpadded row-ring forward shares each tap's weights through LDS
                                   (one barrier per tap); 0 (default): from L1/L2 per wave */
#define FFMP_TUNE_CONV_WGPF 10  /* 1: the weight gradient reads each k-step's operands during the previous
                                   one's MFMAs (two register sets); 0 (default): not */
#define FFMP_TUNE_CONV_BA2 11   /* the 32 -> 64 unpadded row-ring forward (conv2) with each tap's loads pinned
                                   ahead of its MFMAs: 1 = B fragments two taps ahead (rows staged in 2
                                   registers), 2 = one tap ahead; 0 (default): the compiler's schedule */
#define FFMP_TUNE_CONV_MBW 12   /* 32-position blocks per wave of the row-ring forward: 0 (default) = by the
                                   grid-fill model (tiles of 512 / 384 / 256 / 128 positions), 1-4 forced */
#define FFMP_TUNE_CONV_PLANAR 13 /* 1: the row-ring forward keeps each 16-byte channel chunk of a row in a plane of
                                   its own (conflict-free A reads for any first column); 0 (default): padded cells */
#define FFMP_TUNE_CONV_PIN 14   /* 1: the row-ring forward's default launch with each half-trip's loads pinned ahead
                                   of its MFMAs by scheduling barriers; 0 (default): the compiler's schedule */
#define FFMP_TUNE_CONV_WGDMA 15 /* the weight gradient's stages copied by LDS-DMA into two LDS buffers (one barrier
                                   per stage): 0 (default) = with the k-step prefetch where the kernel runs one
                                   workgroup per CU (32 -> 64 channels), 1 = on, 2 = on with the prefetch, 3 = off,
                                   4 = the 32 -> 64 layer with 4 taps per wave, two workgroups per CU */
int32_t ffmp_set_tuning(int32_t key, int32_t value);

/* Host-side, float64: the footprint of ffmp.py:87-94 generalised to G
 * (map_range = G*res).  Writes up to `cap` offsets (cell - G/2); returns the
 * count, or a negative code. */
int ffmp_footprint(int32_t grid, double res, double robot_r,
                   int32_t* di, int32_t* dj, int32_t cap);

/* Reset envs [0,n) (global index env_offset + e) where mask[e] != 0 (mask NULL
 * = all).  initial != 0: episode := 0, else episode += 1.  Writes state, the
 * small obs (g, v=0, t=0, grad, lidar) and the raster record; call ffmp_raster
 * (same mask) afterwards for state_m / potential. */
int ffmp_reset(const ffmp_cfg_t* cfg, int64_t n, int64_t env_offset,
               const uint8_t* mask, int32_t initial,
               ffmp_state_t* state, ffmp_obs_t* obs, void* stream);

/* Injected episodes (an addition within ABI 9: no existing symbol, struct or value changes) — in the
 * reference an episode's start and goal come from outside the env (/episode_manager publishes
 * /start_goal_points, src/train.py:86,88,113-132) and the simulator holds the obstacles.
 * ffmp_set_scenario is ffmp_reset with the sampled episode replaced by the caller's, for envs [0,n)
 * where mask[e] != 0 (mask NULL = all).  DEVICE memory, float64, row e = env e:
 *   pose (n, 3) x, y, yaw      goal (n, 2) world frame
 *   obst (n, K, 4) x, y, vx, vy      obst_r (n, K)       (K = cfg->n_obst; both may be NULL with K == 0)
 *   episode (n) int32: the env's new episode counter, or NULL: episode += 1 (as a masked ffmp_reset)
 * Per selected env, in float64:
 *   every word of pose / goal / obst / obst_r finite, every radius >= 0 and |yaw| <= 1024 (pi_to_pi
 *   is the reference's loop, one turn per trip); otherwise the env is left untouched in every state,
 *   observation and record word and error value 4 is ORed into *state->err
 *   yaw := pi_to_pi(yaw); a disc with r == 0 is a parked disc (it never moves, nothing hits it), as
 *   the sampler's; velocities are stored as given, also with cfg->moving == 0
 *   t := 0; d0, state_g, state_v = 0, state_t = 0, lidar, grad and the raster record (word 10 = 1)
 *   exactly as ffmp_reset computes them from its sampled episode
 * Later auto-resets of the env return to the sampler, keyed (seed, episode + 1, env_offset + e).
 * Call ffmp_raster (same mask) afterwards for state_m / potential, as after ffmp_reset.  The arrays
 * are read with 8-byte loads (no alignment beyond float64's).  pose, goal (or obst, obst_r with
 * K > 0) NULL, negative n or env_offset: FFMP_E_ARG; n == 0: nothing is launched. */
int ffmp_set_scenario(const ffmp_cfg_t* cfg, int64_t n, int64_t env_offset, const uint8_t* mask,
                      const double* pose, const double* goal, const double* obst, const double* obst_r,
                      const int32_t* episode /* NULL ok */, ffmp_state_t* state, ffmp_obs_t* obs,
                      void* stream);

/* One env step for envs [0,n): action[e] in 0..27 (int64, train.py:343-345).
 * Integrates, moves obstacles, lidar, collision/goal/reward/done, truncation,
 * auto-reset (cfg.autoreset), small obs and raster record.  Does NOT raster. */
int ffmp_step_state(const ffmp_cfg_t* cfg, int64_t n, int64_t env_offset,
                    const int64_t* action, ffmp_state_t* state, ffmp_obs_t* obs,
                    ffmp_out_t* out, void* stream);

/* Raster state_m[:,0] (previous frame), state_m[:,1] (current frame) and the
 * potential plane from the raster record (mask NULL = all envs).  Record word 10 is 1 for a
 * record written by a reset (its two frames are identical), else 0. */
int ffmp_raster(const ffmp_cfg_t* cfg, int64_t n, const float* record,
                const uint8_t* mask, ffmp_obs_t* obs, void* stream);

/* ffmp_raster with an explicit launch shape (results are identical for every shape):
 * cells_per_block 0 (default 4096) or a multiple of 1024; flags FFMP_RASTER_*
 * (neither NT nor PLAIN: nontemporal stores for planes of <= 16K cells). */
#define FFMP_RASTER_NT 1     /* nontemporal 16-B stores          */
#define FFMP_RASTER_PLAIN 2  /* plain 16-B stores                */
#define FFMP_RASTER_XCD 4    /* XCD-aware block -> (env, tile) remap */
#define FFMP_RASTER_NEWEST 8 /* temporal stack in place (make_temporal_maps keeps the previous frame,
                                train.py:474-486): write state_m[:,1] (+ potential / flow) for every
                                env but state_m[:,0] only for envs whose record is a first frame
                                (reset: older == newest); the caller points state_m one frame past
                                the previous call's older slot, so [:,0] already holds the previous
                                newest frame */
#define FFMP_RASTER_TILE2 16 /* wave task = a 2 x 128-cell tile instead of 256 consecutive cells */
#define FFMP_RASTER_TILE4 32 /* 4 x 64-cell tile (compact cull box: fewer discs per task)       */
#define FFMP_RASTER_TILE8 64 /* 8 x 32-cell tile; any TILE flag needs G % (256/R) == 0 and blocks
                                of whole R-row bands (cells_per_block % (G*R) == 0 or >= G*G),
                                else the 256-cell chunks are used.  With FFMP_OBS_U8F16 and
                                G % 16 == 0 a wave task is 1024 cells (16 per lane): tiles are
                                R x 1024/R cells and need G % (1024/R) == 0 */
#define FFMP_RASTER_TILE16 256 /* 16 x 16-cell tile (compact 16 cells per lane: 16 x 64) */
#define FFMP_RASTER_NARROW 128 /* FFMP_OBS_U8F16: keep 4 cells per lane (256-cell wave tasks) */
#define FFMP_RASTER_MID8 512   /* FFMP_OBS_U8F16, G % 8 == 0: 8 cells per lane (512-cell wave tasks: an
                                  8-B frame and a 16-B potential store per lane; tiles R x 512/R);
                                  NARROW wins when both are set */
#define FFMP_RASTER_WAVES 1024 /* float32 frames with granule tags, no flow planes (ffmp_raster_ex,
                                  ffmp_step_fused / _cmd): the kernel held to 6 waves per SIMD instead of
                                  the 4 its registers allow.  Identical results.  Ignored without tags,
                                  in the compact format, with flow planes and by ffmp_step_skewed
                                  (ffmp_raster_waves tells). */
#define FFMP_RASTER_DIRECT 2048 /* ffmp_raster_ex, float32 frames with granule tags, no flow planes: the tagged
                                   kernel at 6 waves per SIMD (as FFMP_RASTER_WAVES) in the form whose blocks
                                   use no LDS and no barrier and whose waves make one memory round trip (header
                                   by scalar loads, each lane its own disc, each wave the old tags of its own
                                   tasks).  Row runs, TILE2 and TILE4 in blocks of at most 65,536 cells.
                                   Identical results and tag bytes.  Ignored wherever FFMP_RASTER_WAVES is, with
                                   TILE8 / TILE16, in larger blocks and by the one-launch and skewed steps: the
                                   launch is then the one without the flag (ffmp_raster_direct tells). */
int ffmp_raster_ex(const ffmp_cfg_t* cfg, int64_t n, const float* record,
                   const uint8_t* mask, ffmp_obs_t* obs, int32_t cells_per_block,
                   int32_t flags, void* stream);

/* ffmp_step_state + ffmp_raster_ex in ONE launch (same results): one block per env, whose first
 * wave steps the env and whose 4 waves then raster its whole plane from the record just written
 * (flags as ffmp_raster_ex; cells_per_block is the whole plane, so TILE* needs only
 * G % (256/R) == 0).  The env step's float64 work overlaps other blocks' store streams instead
 * of running as its own launch. */
int ffmp_step_fused(const ffmp_cfg_t* cfg, int64_t n, int64_t env_offset, const int64_t* action,
                    ffmp_state_t* state, ffmp_obs_t* obs, ffmp_out_t* out, int32_t flags, void* stream);

/* The raster of step t and the env step of step t + 1 in ONE launch (round 5): the raster reads
 * record_raster (step t's record, written by the previous launch) and writes obs->state_m /
 * potential as ffmp_raster_ex does (cells_per_block, flags: the same meaning); the env step reads
 * action_next and advances state_next, whose record pointer must be the OTHER record buffer, and
 * writes the small obs (state_g/v/t, grad, lidar) and out of step t + 1.  Nothing either half reads
 * is written by the other, so the env waves' latency chains run beside raster blocks' stores.
 * Within a sequence of steps whose intermediate small outputs nobody reads (a replayed step graph:
 * ffmp_step_state of step 0 into buffer B, then this for t = 0 .. k-2 alternating the buffers, then
 * ffmp_raster_ex of step k-1) every frame, plane, state and record equals k ffmp_step calls.
 * Float32 frames without flow planes only (FFMP_E_ARG otherwise: run the two launches instead). */
int ffmp_step_skewed(const ffmp_cfg_t* cfg, int64_t n, int64_t env_offset, const int64_t* action_next,
                     ffmp_state_t* state_next, ffmp_obs_t* obs, ffmp_out_t* out, const float* record_raster,
                     int32_t cells_per_block, int32_t flags, void* stream);
/* Would ffmp_step_skewed take steps of this config in this obs format with these raster flags
 * (FFMP_RASTER_NT / PLAIN / XCD; NEWEST ignored)?  Runs every check of the launch — the env waves'
 * LDS (static arrays + 4 x envs-per-wave x L beam words) against the device's limit included — and
 * launches nothing.  FFMP_OK, or FFMP_E_ARG with the reason in ffmp_last_error().  A caller that
 * captures skewed step graphs asks this first (FFMPVec.capture) instead of re-deriving the LDS need. */
int ffmp_step_skewed_check(const ffmp_cfg_t* cfg, int32_t format, int32_t flags);

/* Which kernel would ffmp_raster_ex / ffmp_step_fused / ffmp_step_fused_cmd launch for these flags on this
 * obs?  The waves per SIMD the tagged float32 kernel is held to (FFMP_RASTER_WAVES), or 0 for
 * the plain kernel (no such flag, no tags, FFMP_OBS_U8F16 or cfg.flow).  Runs the launches' own checks of cfg
 * and of the tag extension and their own decision, reads no device memory and launches nothing.  Negative:
 * FFMP_E_ARG with the reason in ffmp_last_error(). */
int ffmp_raster_waves(const ffmp_cfg_t* cfg, const ffmp_obs_t* obs, int32_t flags);

/* Would ffmp_raster_ex with these cells_per_block and flags on this obs launch the FFMP_RASTER_DIRECT form?
 * 1: yes, 0: its staged twin or the plain kernel (ffmp_raster_waves tells which).  The launch's own
 * checks and decision; reads no device memory and launches nothing.  Negative: FFMP_E_ARG. */
int ffmp_raster_direct(const ffmp_cfg_t* cfg, const ffmp_obs_t* obs, int32_t cells_per_block, int32_t flags);

/* A scripted reactive controller — no reference counterpart (the reference's actions come from its
 * Q-network, src/train.py:336-347, published as /cmd_vel :665-682) — for closed-loop runs in which
 * step t + 1's action must be computed on the device from step t's observation (benchmarks, demos,
 * smoke tests).  Per env, from obs (the layout ffmp_step / ffmp_raster wrote: state_m's newest frame
 * through its strides and format, state_g):
 *   wi = clamp(rint(orient / 0.2) + 3, 0, 6)               (steer towards the goal)
 *   blocked = any newest-frame cell on the heading ray, rows G/2 + 3 .. G/2 + 3 + round(0.25 / res)
 *             of column G/2, is occupied (> 0)
 *   vi = blocked ? 0 : (dist < 1.0 m ? 1 : 3); blocked with wi == 3 -> wi = 6 (turn in place)
 *   action[e] = 7 * vi + wi   (RobotAction.cmd order, src/gym_ffmp/envs/robot/config.py:25-58)
 * action: (n) int64 device memory.  One thread per env, reads 8 + (look-ahead) cells' bytes. */
int ffmp_policy_reactive(const ffmp_cfg_t* cfg, int64_t n, const ffmp_obs_t* obs, int64_t* action, void* stream);

/* ffmp_step_state + ffmp_raster. */
int ffmp_step(const ffmp_cfg_t* cfg, int64_t n, int64_t env_offset,
              const int64_t* action, ffmp_state_t* state, ffmp_obs_t* obs,
              ffmp_out_t* out, void* stream);

/* Continuous velocity commands (ABI 9) — the reference's action space is the Box
 * [0, -0.6] .. [0.6, 0.6] of (v, w) (src/gym_ffmp/envs/ffmp.py:29-32) and cmd_vel_publisher sends
 * any such Twist (src/train.py:134-143); the 28 action ids are one table over it.  cmd: (n, 2)
 * float64 DEVICE memory, row e = {v, w} of env e, 16-byte aligned (read as one 16-byte load per env).
 * Per env:
 *   v or w NaN           -> the env runs (0.0, 0.0) and error value 2 is ORed into *state->err
 *   v = v < 0.0 ? 0.0 : (v > 0.6 ? 0.6 : v)        (the bounds are cmd[0] and cmd[27]; +-inf clips,
 *   w = w < -0.6 ? -0.6 : (w > 0.6 ? 0.6 : w)       -0.0 passes through)
 * and the step from the unicycle integrator on is that of the action-id entry points: a command
 * equal to the float64 table entry of action id a gives the bits ffmp_step_state gives for a.
 * ffmp_step_state_cmd / ffmp_step_fused_cmd / ffmp_step_cmd are ffmp_step_state / ffmp_step_fused /
 * ffmp_step with that command source (every other argument as there).  cmd NULL or not 16-byte
 * aligned: FFMP_E_ARG; n == 0: nothing is launched.  (ffmp_step_skewed takes ids only: it needs the
 * actions a step ahead, which a closed loop over commands never has.) */
int ffmp_step_state_cmd(const ffmp_cfg_t* cfg, int64_t n, int64_t env_offset, const double* cmd,
                        ffmp_state_t* state, ffmp_obs_t* obs, ffmp_out_t* out, void* stream);
int ffmp_step_fused_cmd(const ffmp_cfg_t* cfg, int64_t n, int64_t env_offset, const double* cmd,
                        ffmp_state_t* state, ffmp_obs_t* obs, ffmp_out_t* out, int32_t flags, void* stream);
int ffmp_step_cmd(const ffmp_cfg_t* cfg, int64_t n, int64_t env_offset, const double* cmd,
                  ffmp_state_t* state, ffmp_obs_t* obs, ffmp_out_t* out, void* stream);

/* A scripted field follower — no reference counterpart (the reference's commands come from its
 * Q-network through cmd_vel_publisher, src/train.py:134-143, inside the Box of
 * src/gym_ffmp/envs/ffmp.py:29-32) — that descends the potential field: per env, from obs->grad
 * (float32, ego frame, x = heading), in float64 and in this order:
 *   gx, gy = grad[0], grad[1];  m2 = gx*gx + gy*gy
 *   m2 not > 0, or not finite:  cmd = (0, 0)
 *   else  m = sqrt(m2);  dx = -gx / m;  dy = -gy / m          (unit descent direction)
 *         w = dy / cfg->dt, then w < -0.6 ? -0.6 : (w > 0.6 ? 0.6 : w)
 *         if dx < 0:  w = dy >= 0 ? 0.6 : -0.6                 (descent points behind: turn on the spot)
 *         v = 0.6 * (dx > 0 ? dx : 0.0)
 * cmd: (n, 2) float64 device memory, 16-byte aligned — what the *_cmd steps read.  obs->grad or cmd
 * NULL, cmd misaligned: FFMP_E_ARG; cfg->dt == 0 (w divides by it): FFMP_E_CFG; n == 0: nothing is
 * launched.  One lane per env. */
int ffmp_policy_field(const ffmp_cfg_t* cfg, int64_t n, const ffmp_obs_t* obs, double* cmd, void* stream);

/* A navigation field (an addition within ABI 9: no existing symbol, struct or value changes) — no
 * reference counterpart (the reference plans with its Q-network, src/train.py:336-347; it has no
 * path planner): the flow field of the pathfinding sense over the newest ego frame.  Per env, the
 * cost-to-go from the goal cell over the traversable cells (an integration field), the direction
 * per cell, and a follower that tracks the descent path from the robot cell.  All arithmetic is
 * integer unless stated.  Inputs per env: the newest occupancy frame F (G x G through obs->state_m,
 * its strides and format; row i = ego x = heading, column j = ego y; robot cell c = (G/2, G/2)) and
 * the goal in the ego frame g = goal_ego[e * goal_stride + 0..1], float32 (FFMPVec: record words 8..9).
 * Cell classes:
 *   occ[i][j]  = F[i][j] > 0
 *   hard[i][j] = any occ[i + di][j + dj] over the cfg->n_foot footprint offsets (offsets that fall
 *                outside the grid are ignored)
 *   zone       = hard dilated `margin` times by the 3 x 3 neighbourhood
 *   goal cell  q = clamp(rint(((double)g + (double)half_f) / (double)res_f), 0, G - 1) per axis
 *                (float64, rint half to even); a non-finite g makes the env unreachable (below)
 *   then hard[c] = hard[q] = false;  soft = zone & ~hard (a cleared cell counts as soft)
 *   pen(a) = soft[a] ? soft_pen : 0
 * Neighbours, in this order k = 0..7: (1,0) (-1,0) (0,1) (0,-1) (1,1) (1,-1) (-1,1) (-1,-1), weight
 * w_k = 5 for k < 4, else 7.  A diagonal move a -> a + (di, dj) is allowed only if neither
 * a + (di, 0) nor a + (0, dj) is hard (no corner cutting).
 * Cost-to-go d (uint16; 65535 = hard or unreachable): d[q] = 0; for every other non-hard cell
 *   d[a] = pen(a) + min_k(d[a + k] + w_k) over in-grid, allowed neighbours with d < 65535,
 * a candidate accepted only if it is <= 65534.  The fixed point is unique (prefixes of a shortest
 * path are shorter), so the relaxation order does not show in the bits.
 * Direction dir[a] (uint8): the k minimising d[a + k] + w_k under the same rules, the lowest k
 * winning ties; 8 at q; 255 where d[a] == 65535.
 * Robot outputs: geo_cost = d[c], or -1 if it is 65535.  From c follow dir for at most `lookahead`
 * moves, stopping at q or where no neighbour qualifies: target = (ti - G/2, tj - G/2) of the cell
 * reached.  An unreachable env (geo_cost -1) gets target (0, 0) and cmd (0, 0); an env with a
 * non-finite g also gets cost 65535 and dir 255 in every cell.
 * Follower, float64, in this order:
 *   dx = target[0];  dy = target[1];  m2 = dx*dx + dy*dy;   m2 == 0: cmd = (0, 0)
 *   else  m = sqrt(m2);  ux = dx / m;  uy = dy / m
 *         w = uy / cfg->dt, then w < -0.6 ? -0.6 : (w > 0.6 ? 0.6 : w)    (ffmp_policy_field's compares)
 *         if ux < 0:  w = uy >= 0 ? 0.6 : -0.6
 *         v = 0.6 * (ux > 0 ? ux : 0.0)
 *         if fabs(uy) > turn_sin:  v = 0.0      (turn on the spot: track the path, do not cut it)
 * Defaults of the Python surface: margin 2, soft_pen 40, lookahead 4, turn_sin 0.25.
 * cfg gives grid, the footprint, res_f, half_f and dt.  cost, dir (n, G, G), target (n, 2),
 * geo_cost (n) and cmd (n, 2; what the *_cmd steps read) are DEVICE memory, each written only when
 * non-NULL.  One workgroup per env holds the whole plane in LDS, so 8 <= G <= 256, G % 4 == 0.
 * FFMP_E_ARG, with a message and before any HIP call, for: G outside that range; margin outside
 * 0..8; soft_pen outside 0..16384; lookahead outside 1..64; turn_sin NaN or negative; obs,
 * obs->state_m or goal_ego NULL; goal_stride < 2; cmd not 16-byte, cost not 8-byte or dir not 4-byte
 * aligned; an unknown obs format; n < 0.  n == 0: nothing is launched.  Obstacle velocities are not
 * looked at (a static plan over the newest frame), and the follower is stateless.
 * cmd given with cfg->dt == 0 (the follower's turn rate divides by it): FFMP_E_CFG; the planes alone
 * need no dt.
 * ffmp_nav_field_check: the checks that need no pointer (shape, format, knobs, LDS budget), no launch. */
int ffmp_nav_field(const ffmp_cfg_t* cfg, int64_t n, const ffmp_obs_t* obs,
                   const float* goal_ego, int64_t goal_stride /* floats between envs */,
                   int32_t margin, int32_t soft_pen, int32_t lookahead, double turn_sin,
                   uint16_t* cost /* (n,G,G) or NULL */, uint8_t* dir /* (n,G,G) or NULL */,
                   int32_t* target /* (n,2) or NULL */, int32_t* geo_cost /* (n) or NULL */,
                   double* cmd /* (n,2), 16-B aligned, or NULL */, void* stream);
int ffmp_nav_field_check(const ffmp_cfg_t* cfg, int32_t format, int32_t margin, int32_t soft_pen, int32_t lookahead);

/* The same field on grids up to 512 x 512 (an addition within ABI 9: no existing symbol, struct or
 * value changes): the SPEC above ffmp_nav_field, every output bit for bit what it defines — the
 * fixed point is unique, so the tiling does not show.  8 <= G <= 512, G % 4 == 0.
 * Tiling: the cost plane of an env lives in global memory (the caller's cost + e G^2 when cost is
 * given, else in the workspace) and is relaxed a tile of `tile` x `tile` cells at a time through
 * LDS, each tile with a one-cell halo that is read and never relaxed; a tile whose border changed
 * makes the neighbours that see the change due again, until no tile is due.  tile: 0 = the default,
 * 256; otherwise a multiple of 32 in [32, 256] (a tile larger than the grid is cut to it).
 * Schedule: a persistent grid of `slots` workgroups, workgroup b planning envs b, b + slots, ...;
 * slots = min(n, CUs x resident workgroups per CU), at most 2048.  No workgroup waits on another.
 * Workspace: DEVICE memory, 256-byte aligned, slots x per-slot bytes — per slot the hard and soft
 * masks of the grid (2 x G x ceil(G / 32) words, rounded up to 256 bytes) and, when cost is NULL,
 * a plane of G^2 uint16 (rounded likewise).  ffmp_nav_field_tiled_workspace writes that product to
 * *bytes for the current device, the same slot count the launch uses; with_cost != 0: the calls
 * will pass cost.  Without a HIP device it answers with the bound min(n, 2048) slots.  The contents
 * need not survive between calls; calls that may run concurrently need a workspace each.
 * FFMP_E_ARG, with a message and before any HIP call, for: everything ffmp_nav_field refuses (with
 * the grid range above); a tile that is neither 0 nor a multiple of 32 in [32, 256]; workspace NULL,
 * not 256-byte aligned, or smaller than one slot (smaller than slots x per-slot bytes: refused once
 * the device's slot count is known, before the launch).  n == 0: nothing is launched.
 * ffmp_nav_field_tiled_check: the checks that need no pointer (shape, format, knobs, tile, LDS
 * budget), no launch. */
int ffmp_nav_field_tiled(const ffmp_cfg_t* cfg, int64_t n, const ffmp_obs_t* obs,
                         const float* goal_ego, int64_t goal_stride /* floats between envs */,
                         int32_t margin, int32_t soft_pen, int32_t lookahead, double turn_sin,
                         uint16_t* cost /* (n,G,G) or NULL */, uint8_t* dir /* (n,G,G) or NULL */,
                         int32_t* target /* (n,2) or NULL */, int32_t* geo_cost /* (n) or NULL */,
                         double* cmd /* (n,2), 16-B aligned, or NULL */,
                         int32_t tile, void* workspace, size_t workspace_bytes, void* stream);
int ffmp_nav_field_tiled_check(const ffmp_cfg_t* cfg, int32_t format, int32_t margin, int32_t soft_pen, int32_t lookahead,
                               int32_t tile);
int ffmp_nav_field_tiled_workspace(const ffmp_cfg_t* cfg, int64_t n, int32_t tile, int with_cost, size_t* bytes);

/* Sensor-visible occupancy frames (an addition within ABI 9: no existing symbol, struct or value
 * changes) — stands in for what the reference's external, sensor-driven BEV node shows
 * (/bev_flow_estimator -> /bev/temporal_bev_image, src/train.py:116-121): an image that cannot
 * contain what an obstacle hides from the robot.  That node is not in the reference's repository, so
 * there is no reference counterpart to pin this against [unpinned]; the SPEC below is the definition.
 * Inputs per env: the raster record (FFMP_REC_HDR + 12K floats) and cfg.  Two frames: the older one
 * (header words 4..7 and the K previous-frame discs) and the newest one (header words 0..3 and the K
 * current-frame discs).  The sensor sits at the ego origin.  All arithmetic is float32, every
 * expression evaluated left to right as written (products first, then the sum; no FMA contraction);
 * comparisons as written, so a NaN compares false.  Per frame and cell (i, j):
 *   ex = (float)i * res_f - half_f;  ey = (float)j * res_f - half_f      (the raster's cell coordinates)
 *   occ = the raster's occupancy of (ex, ey) under this frame's header and discs
 *         (outside the world, or dx*dx + dy*dy <= r2_k for any disc k)
 *   b   = ex*ex + ey*ey
 *   far = b > rr,   rr = max_range * max_range                           (max_range = +inf: never)
 *   for each disc k = {ox, oy, r2, r} of this frame with r2 > 0:
 *       dx = ex - ox;  dy = ey - oy;  inside = dx*dx + dy*dy <= r2
 *       a  = ex*ox + ey*oy
 *       oo = ox*ox + oy*oy
 *       q  = oo - r2
 *       hides_k = !inside && ( q <= 0  ||  ( a > 0 && a < b && oo*b - a*a <= r2*b ) )
 *   value = (far || any hides_k) ? unknown : (occ ? 255 : 0)
 * q <= 0: the sensor is inside disc k and everything outside that disc is hidden.  The last test is
 * "the segment from the sensor to the cell centre passes within r of the disc's centre" without a
 * division or a square root.  A cell inside a disc is never hidden by that disc: a disc shows whole
 * unless another disc hides it.  Parked discs (r = 0) hide nothing.  The world's walls hide nothing:
 * the free world is convex, so what lies beyond a wall is outside the world and stays 255.
 * Wherever the value is not `unknown` it is the value the raster's frame (state_m) holds for the cell.
 * A reset record (word 10 = 1) holds the same header and discs twice, so its two frames come out equal.
 * unknown: a byte, 0..255 (0: the image of a hit-based estimator, hidden things are simply absent).
 * format: FFMP_OBS_F32 writes (float)value, FFMP_OBS_U8F16 the byte.
 * record: DEVICE memory, env e's record at record + e * record_stride floats (4-byte loads).
 * out_older / out_newest: DEVICE memory, either may be NULL (that frame is not computed); element
 * (e, i, j) at e * out_env_stride + i*G + j elements — a contiguous (N,2,G,G) block is newest =
 * older + G*G with stride 2 G*G, a (N,G,G) plane has stride G*G, a slot-major window its own.  Each
 * lane stores 4 cells at once, so the pointers must be 16-byte (F32) or 4-byte (U8F16) aligned and
 * out_env_stride a multiple of 4 elements; anything else is refused (there is no scalar-store path).
 * mask: (n) bytes or NULL = all; an env with mask[e] == 0 keeps its output cells (as ffmp_raster_ex).
 * flags: FFMP_VISIBLE_NOCULL runs every disc for every cell instead of the discs a wave task's box
 * can be inside of or shadowed by — the same bits, for checking the culls against.
 * FFMP_E_ARG, with a message and before any HIP call, for: grid outside 8..4096 or not a multiple of
 * 4; n_obst outside 0..FFMP_MAX_OBST; an unknown format; unknown outside 0..255; max_range NaN or
 * negative; unknown flag bits; record NULL; record_stride < FFMP_REC_HDR + 12K; both outputs NULL;
 * out_env_stride < G*G; a misaligned output or stride; n < 0 or too large for one launch.
 * n == 0: nothing is launched.
 * ffmp_visible_frames_check: the checks that need no pointer (shape, format, knobs), no launch. */
#define FFMP_VISIBLE_NOCULL 1
int ffmp_visible_frames(const ffmp_cfg_t* cfg, int64_t n, const float* record, int64_t record_stride,
                        const uint8_t* mask, void* out_older, void* out_newest, int64_t out_env_stride,
                        int32_t format, int32_t unknown, float max_range, int32_t flags, void* stream);
int ffmp_visible_frames_check(const ffmp_cfg_t* cfg, int32_t format, int32_t unknown, float max_range, int32_t flags);

/* Occupancy frames built from the lidar scan (an addition within ABI 9: no existing symbol, struct or
 * value changes) — the inverse sensor model: the map a robot can make of its own /scan, where
 * ffmp_visible_frames still reads the ground-truth disc list.  The reference's BEV node builds its
 * image from sensor data (src/train.py:87,116-121,145-150) but is not in its repository, so there is
 * no reference counterpart to pin this against [unpinned]; the SPEC below is the definition.
 * Inputs per env:
 *   ranges  a row of L float32 ranges in the env's lidar convention: beam l at angle -pi + l*2pi/L in
 *           the robot frame; +inf = no return, -inf = the origin is inside a disc, NaN = no data.
 *   u       the sector table (L, 2) float32, supplied by the caller: u[m] is the float32 rounding of
 *           (cos, sin) of the float64 angle -pi + (m - 1/2)*2pi/L (math.cos / math.sin on the host;
 *           config.sector_table(L)).  Sector m is the cone of beam m.
 * All arithmetic is float32, every expression evaluated left to right as written (products first,
 * then the sum; no FMA contraction); comparisons as written, so a NaN compares false.  Per cell (i, j):
 *   ex = (float)i * res_f - half_f;  ey = (float)j * res_f - half_f      (the raster's cell coordinates)
 *   H  = (L + 1) / 2                                                      (integer)
 *   c0 = u[0].x*ey - u[0].y*ex
 *   (lo, hi) = c0 >= 0 ? (0, H) : (H - 1, L)
 *   while hi - lo > 1:  mid = (lo + hi) >> 1;  t = u[mid].x*ey - u[mid].y*ex;  if t >= 0: lo = mid  else: hi = mid
 *   r  = ranges[lo]
 *   b  = ex*ex + ey*ey;   mm = range_max_f * range_max_f;   lo_r = r - th;   hi_r = r + th
 *   known = (b <= mm) && (r > 0)                       (NaN, 0, negative, -inf: no data for this cone)
 *   free  = (lo_r > 0) && (b < lo_r*lo_r)
 *   occ   = b <= hi_r*hi_r
 *   value = !known ? unknown : free ? 0 : occ ? 255 : unknown
 * The procedure is the definition, not "the nearest beam by atan2": where a cell centre lies exactly
 * on a cone boundary the two differ, by tens of cells and depending on how the atan2 form breaks
 * its ties (142 of the 4,096 cell centres lie within 1e-4 rad of a boundary at G = 64, L = 180).
 * unknown: a byte, 0..255.  thickness (th): the hit's thickness in metres, >= 0 and finite (res gives
 * an arc two cells thick with no radial holes).  range_max: > 0 or +inf; a +inf range gives free
 * space out to range_max.  format: FFMP_OBS_F32 writes (float)value, FFMP_OBS_U8F16 the byte.
 * n_beams: L, 1..FFMP_MAX_BEAMS — an argument, not cfg.n_beams (which is not looked at): a caller may
 * bring a scan to an env built with L = 0.
 * ranges: DEVICE memory, env e's row at ranges + e * ranges_stride floats.  sectors: DEVICE memory,
 * 2L floats.  mask: (n) bytes or NULL = all; an env with mask[e] == 0 keeps all its cells, older included.
 * The temporal pair (make_temporal_maps, train.py:474-486): first is (n) bytes or NULL.
 *   out_older given and (first == NULL or first[e] != 0, or out_newest == NULL): older gets the new value too;
 *   out_older given and first[e] == 0: each cell of older gets the value out_newest held for that cell
 *       before the call — the lane that reads the cell is the lane that then stores it;
 *   out_older == NULL: only newest is written.
 * out_older / out_newest: DEVICE memory, addressed as in ffmp_visible_frames: element (e, i, j) at
 * e * out_env_stride + i*G + j elements; 16-byte (F32) or 4-byte (U8F16) aligned pointers and a stride
 * that is a multiple of 4 elements and >= G*G; anything else is refused (there is no scalar-store
 * path).  No plane of one frame may overlap a plane of the other.
 * flags: FFMP_SCAN_PLAIN runs the SPEC's bisection for every cell.  Without it a lane's second to
 * fourth cells start from the previous cell's cone: they look for "t(lo) >= 0 and t(lo + 1) < 0"
 * inside the cell's own half-turn at that cone and its two neighbours, and bisect only when none of
 * the three has it — the same bits, the predicate being monotone in m inside a half-turn
 * (csrc/ffmp_scan.hip).
 * FFMP_E_ARG, with a message and before any HIP call, for: grid outside 8..4096 or not a multiple of
 * 4; n_beams outside 1..FFMP_MAX_BEAMS; an unknown format; unknown outside 0..255; thickness NaN,
 * negative or infinite; range_max NaN or <= 0; unknown flag bits; ranges or sectors NULL;
 * ranges_stride < n_beams; both outputs NULL; out_env_stride < G*G; a misaligned output or stride;
 * overlapping older and newest planes (closer than G*G elements, across envs included); n < 0 or too
 * large for one launch.  n == 0: nothing is launched.
 * ffmp_scan_frames_check: the checks that need no pointer (shape, format, knobs), no launch. */
#define FFMP_SCAN_PLAIN 1
int ffmp_scan_frames(const ffmp_cfg_t* cfg, int64_t n, const float* ranges, int64_t ranges_stride, int32_t n_beams,
                     const float* sectors, const uint8_t* mask, const uint8_t* first,
                     void* out_older, void* out_newest, int64_t out_env_stride, int32_t format, int32_t unknown,
                     float thickness, float range_max, int32_t flags, void* stream);
int ffmp_scan_frames_check(const ffmp_cfg_t* cfg, int32_t n_beams, int32_t format, int32_t unknown,
                           float thickness, float range_max, int32_t flags);

/* The accumulated scan map (an addition within ABI 9: no existing symbol, struct or value changes) —
 * log-odds over time with ego-motion compensation: ffmp_scan_frames has no memory, this keeps one.
 * As ffmp_scan_frames it has no reference counterpart (the BEV node is outside the reference's
 * repository) [unpinned]; the SPEC below is the definition.
 * State: one int8 plane per env, M (G x G): the cell's log-odds in integer units — 0 nothing known,
 * positive occupied, negative free.  The map is ego-centric like every other plane here (row i is
 * ego x, column j is ego y, the robot at (G/2, G/2)), so it is re-sampled into the new ego frame on
 * every update.
 * Ego motion, per env: float64 from eight float32 words, then rounded to float32.
 *   pose_now = {px1, py1, c1, s1};  pose_prev = {px0, py0, c0, s0}       (the layout of record words 0..3)
 *   dx = px1 - px0;  dy = py1 - py0
 *   cr = c0*c1 + s0*s1
 *   sr = c0*s1 - s0*c1
 *   tx = (c0*dx + s0*dy) / double(res_f)
 *   ty = (c0*dy - s0*dx) / double(res_f)
 * An env restarts (its prior is 0 everywhere) if its `first` byte is non-zero, or if any of the four
 * rounded values is not finite.
 * Per cell (i, j): float32, no FMA contraction, operation order as written.
 *   a = float(i - G/2);  b = float(j - G/2)
 *   u = (cr*a - sr*b) + tx
 *   v = (sr*a + cr*b) + ty
 *   ru = rintf(u);  rv = rintf(v)                                         (rounding half to even)
 *   inside = ru >= -G/2 && ru <= G/2 - 1, and the same for rv             (float compares: a NaN is outside)
 *   prior = M_in[(int)ru + G/2][(int)rv + G/2] if inside and the env does not restart, else 0
 * (a nearest-neighbour gather).  The class of the cell comes from this scan: exactly ffmp_scan_frames'
 * classification with the same thickness and range_max (that SPEC is unchanged, the bisection included):
 *   free = known && free;  hit = known && !free && occ;  no information otherwise.
 * The `unknown` byte plays no part in this step.  Update: int32 arithmetic, stored as int8.
 *   hit:            M_out = clamp(prior + l_hit, -l_max, l_max)
 *   free:           M_out = clamp(prior - l_free, -l_max, l_max)
 *   no information: M_out = prior - sgn(prior) * min(|prior|, decay)
 * Frame (optional, FFMP_OBS_F32 writes (float)value, FFMP_OBS_U8F16 the byte):
 *   value = M_out >= occ_thr ? 255 : M_out <= -free_thr ? 0 : unknown
 * mask: (n) bytes or NULL = all; an env with mask[e] == 0 gets M_out = M_in copied cell for cell, with
 * no warp, and its frame is not written.  first: (n) bytes, or NULL = no env restarts on that account.
 * Knobs: 0 <= l_hit, l_free, decay <= 127; 1 <= l_max, occ_thr, free_thr <= 127.  unknown, thickness,
 * range_max, n_beams, ranges, sectors and FFMP_SCAN_PLAIN (no search shortcut, the same bits) are as
 * in ffmp_scan_frames.
 * Known limits: a moving obstacle leaves a trail of stale hits until the beam sweeps it free again or
 * decay fades it; nearest-neighbour re-sampling on every update jitters edges by up to a cell.
 * pose_now / pose_prev: DEVICE memory, env e's four words at pose + e * stride floats (stride >= 4).
 * map_in / map_out: DEVICE memory, cell (e, i, j) at e * map_env_stride + i*G + j bytes; 4-byte
 * aligned, map_env_stride a multiple of 4 and >= G*G.  They are different buffers, because the gather
 * reads arbitrary cells: overlapping planes are refused, by the test ffmp_scan_frames applies to its
 * pair.  frame_out: NULL, or addressed and aligned as ffmp_scan_frames' outputs with frame_env_stride.
 * FFMP_E_ARG, with a message and before any HIP call, for: everything ffmp_scan_frames_check refuses;
 * a knob out of range; ranges, sectors, pose_now, pose_prev, map_in or map_out NULL; a stride that is
 * too small; a misaligned map plane, frame or stride; overlapping map_in and map_out planes; n < 0 or
 * too large for one launch.  n == 0: nothing is launched.
 * ffmp_scan_map_check: the checks that need no pointer (shape, format, knobs), no launch. */
int ffmp_scan_map(const ffmp_cfg_t* cfg, int64_t n, const float* ranges, int64_t ranges_stride, int32_t n_beams,
                  const float* sectors, const float* pose_now, int64_t pose_now_stride, const float* pose_prev,
                  int64_t pose_prev_stride, const uint8_t* mask, const uint8_t* first, const int8_t* map_in,
                  int8_t* map_out, int64_t map_env_stride, void* frame_out, int64_t frame_env_stride, int32_t format,
                  int32_t unknown, float thickness, float range_max, int32_t l_hit, int32_t l_free, int32_t l_max,
                  int32_t decay, int32_t occ_thr, int32_t free_thr, int32_t flags, void* stream);
int ffmp_scan_map_check(const ffmp_cfg_t* cfg, int32_t n_beams, int32_t format, int32_t unknown, float thickness,
                        float range_max, int32_t l_hit, int32_t l_free, int32_t l_max, int32_t decay, int32_t occ_thr,
                        int32_t free_thr, int32_t flags);

/* The world-fixed scan map (an addition within ABI 9: no existing symbol, struct or value changes) —
 * ffmp_scan_map re-samples its plane into the new ego frame on every update (edges jitter, and what
 * leaves the G x G window is forgotten); this map has one log-odds cell per WORLD cell, is updated in
 * place and never re-sampled, and is cut out and rotated into the ego frame only when asked
 * (ffmp_world_frame).  No reference counterpart [unpinned]; the SPEC below is the definition.
 * State: one int8 plane per env, M (Wc x Wc), Wc = `cells` a multiple of 4 in [8, 2048]: cell (p, q) of
 * env e at e * map_env_stride + p*Wc + q bytes; the pointer 4-byte aligned, map_env_stride a multiple of 4
 * and >= Wc*Wc.  Row p is world x, column q is world y.  World cell centres, float32:
 *   wh_f = (float)(Wc * res / 2)                       (cfg.res, float64 on the host, then rounded)
 *   wx = (float)p * res_f - wh_f;  wy = (float)q * res_f - wh_f
 * so the plane is centred on the world's origin and covers [-wh_f, wh_f).
 *
 * ffmp_world_map: the update, in place, one launch.  ranges, ranges_stride, n_beams, sectors, thickness,
 * range_max, the knobs l_hit, l_free, l_max, decay (their ranges included) and FFMP_SCAN_PLAIN (no search
 * shortcut, the same bits) are as in ffmp_scan_map.  pose: DEVICE memory, env e's four float32 words
 * {px, py, c, s} (record words 0..3: position, cos yaw, sin yaw) at pose + e * pose_stride floats,
 * pose_stride >= 4.  Per world cell (p, q): float32, no FMA contraction, operation order as written.
 *   dx = wx - px;  dy = wy - py
 *   ex = c*dx + s*dy;  ey = c*dy - s*dx
 * The class of the cell is ffmp_scan_frames' classification verbatim with these (ex, ey) in place of the
 * grid's cell coordinates: the half-turn from c0, the bisection over the sector table, r, b, known, free,
 * occ.  Update, int32 arithmetic, stored as int8:
 *   not known (b > range_max^2, or no data in its cone):  M unchanged
 *   free:                 M = clamp(M - l_free, -l_max, l_max)
 *   occ and not free:     M = clamp(M + l_hit, -l_max, l_max)
 *   known, neither:       M = M - sgn(M) * min(|M|, decay)
 * Not-known cells keep their value, so an implementation may visit any superset of the sensor disc's
 * bounding box (the kernel: that box clipped to the plane, columns rounded out to multiples of 4; the
 * whole plane for a range_max whose float32 square is +inf) and gives the same bits.
 * Per env: mask[e] == 0 (mask: (n) bytes or NULL = all) leaves every byte of the env unchanged.
 * first[e] != 0 (first: (n) bytes or NULL = none) zeroes the env's whole plane before the update.  A
 * non-finite pose word leaves the plane as it is — as it is after the zeroing, for an env with first set.
 * FFMP_E_ARG, with a message and before any HIP call, for: cfg NULL or res_f not > 0; cells outside
 * 8..2048 or not a multiple of 4; n_beams outside 1..FFMP_MAX_BEAMS; thickness NaN, negative or infinite;
 * range_max NaN or <= 0; a knob out of range; unknown flag bits; ranges, sectors, pose or map NULL;
 * ranges_stride < n_beams; pose_stride < 4; map_env_stride < Wc*Wc; a misaligned map or stride; n < 0 or
 * too large for one launch.  n == 0: nothing is launched.
 * ffmp_world_map_check: the checks that need no pointer (shape, knobs), no launch.
 *
 * ffmp_world_frame: the ego view, one launch, read-only on the map.  Per ego cell (i, j), float32 as above:
 *   ex = (float)i * res_f - half_f;  ey = (float)j * res_f - half_f      (the raster's cell coordinates)
 *   wx = (c*ex - s*ey) + px;  wy = (s*ex + c*ey) + py
 *   fp = rintf((wx + wh_f) / res_f);  fq = rintf((wy + wh_f) / res_f)     (rounding half to even)
 *   inside = fp >= 0 && fp <= Wc - 1 && fq >= 0 && fq <= Wc - 1           (float compares: a NaN is outside)
 *   value = !inside ? outside : M[fp][fq] >= occ_thr ? 255 : M[fp][fq] <= -free_thr ? 0 : unknown
 * outside, unknown: bytes 0..255; 1 <= occ_thr, free_thr <= 127.  An env with a non-finite pose word gets
 * a frame of `unknown` only.  frame_out: FFMP_OBS_F32 writes (float)value, FFMP_OBS_U8F16 the byte;
 * addressed and aligned as ffmp_scan_frames' outputs with frame_env_stride (16- or 4-byte aligned, the
 * stride a multiple of 4 elements and >= G*G).
 * FFMP_E_ARG, with a message and before any HIP call, for: cfg NULL or res_f not > 0; cells or grid out of
 * range; an unknown format; unknown or outside outside 0..255; a threshold out of range; pose, map or
 * frame_out NULL; a stride that is too small; a misaligned frame or stride; a frame whose bytes overlap
 * the map's; n < 0 or too large for one launch.  n == 0: nothing is launched.
 * ffmp_world_frame_check: the checks that need no pointer (shape, format, knobs), no launch. */
int ffmp_world_map(const ffmp_cfg_t* cfg, int64_t n, const float* ranges, int64_t ranges_stride, int32_t n_beams,
                   const float* sectors, const float* pose, int64_t pose_stride, const uint8_t* mask, const uint8_t* first,
                   int8_t* map, int64_t map_env_stride, int32_t cells, float thickness, float range_max, int32_t l_hit,
                   int32_t l_free, int32_t l_max, int32_t decay, int32_t flags, void* stream);
int ffmp_world_map_check(const ffmp_cfg_t* cfg, int32_t n_beams, int32_t cells, float thickness, float range_max,
                         int32_t l_hit, int32_t l_free, int32_t l_max, int32_t decay, int32_t flags);
int ffmp_world_frame(const ffmp_cfg_t* cfg, int64_t n, const float* pose, int64_t pose_stride, const int8_t* map,
                     int64_t map_env_stride, int32_t cells, void* frame_out, int64_t frame_env_stride, int32_t format,
                     int32_t unknown, int32_t outside, int32_t occ_thr, int32_t free_thr, void* stream);
int ffmp_world_frame_check(const ffmp_cfg_t* cfg, int32_t cells, int32_t format, int32_t unknown, int32_t outside,
                           int32_t occ_thr, int32_t free_thr);

/* Scan-to-map matching (an addition within ABI 9: no existing symbol, struct or value changes) — the
 * localisation half of occupancy-grid mapping: the scan's endpoints are scored against ffmp_world_map's plane
 * at every whole-cell shift (a, b), |a|, |b| <= R, and every rotation step k, |k| <= T, round the prior pose
 * (from odometry), and the best candidate's pose is what the scan is then integrated at.  An exhaustive
 * correlative search with integer scores.  No reference counterpart [unpinned]; the SPEC below is the
 * definition.  One launch, read-only on the map.
 * ranges, ranges_stride, n_beams = L (1..FFMP_MAX_BEAMS), range_max (> 0 or +inf): ffmp_scan_frames' conventions.
 * beams: DEVICE (L, 2) float32, the rounding of {cos, sin}(-pi + l*2pi/L) computed in float64 (the caller's
 * table).  pose, pose_stride, mask, map, map_env_stride, cells = Wc: exactly ffmp_world_map's, the map const.
 * turns: DEVICE (2T + 1, 2) float32 {cos, sin} of (k - T) * dtheta, computed on the host in float64 and
 * rounded; entry T is (1, 0).  n_turns = T in 0..32, radius = R in 0..16 (cells), min_valid >= 0, min_gain >= 0.
 * Arithmetic: float32, no FMA contraction, operation order as written; a NaN compares false.
 * Per beam l:
 *   r = ranges[l];  valid_l = (r > 0) && (r <= range_max) && (r <= FLT_MAX)
 *   bx = r*beams[l].x;  by = r*beams[l].y
 * Per rotation k in -T..T, with (rc, rs) = turns[k + T]:
 *   ck = c*rc - s*rs;  sk = s*rc + c*rs
 *   wx = (ck*bx - sk*by) + px;  wy = (sk*bx + ck*by) + py
 *   fp = rintf((wx + wh_f) / res_f);  fq = rintf((wy + wh_f) / res_f)     (ffmp_world_frame's cell rule)
 *   on_l,k = valid_l && fp >= -R && fp <= Wc-1+R && fq >= -R && fq <= Wc-1+R
 * float compares; fp and fq are converted to int only where on_l,k holds.  An env with a non-finite pose word
 * has no beam on.  Score, int32:
 *   S(k, a, b) = sum over l with on_l,k and (fp+a, fq+b) inside 0..Wc-1 of M[fp+a][fq+b],   a, b in -R..R
 * — an occupied cell rewards an endpoint, a free cell penalises it, unknown cells and cells off the plane count 0.
 * Winner: the largest S; ties go to the smaller a*a + b*b, then the smaller |k|, then the smaller k, then the
 * smaller a, then the smaller b — a total order, so the order of the reduction does not show.
 * Gate: valid = the number of beams with valid_l.  status = 0 if a pose word is non-finite, or valid < min_valid,
 * or S_best - S(0,0,0) < min_gain, or the winner is (0, 0, 0); otherwise status = 1.
 * Outputs, DEVICE memory, each written only when non-NULL (not all three NULL):
 *   pose_out (n, 4) float32, 16-byte aligned: status 0 — the four prior words copied bit for bit; status 1 —
 *     {px + (float)a*res_f, py + (float)b*res_f, ck, sk} of the winner (the layout ffmp_world_map takes)
 *   info (n, 8) int32, 16-byte aligned: {status, k, a, b, S_best, S(0,0,0), valid, 0}; k, a, b are 0 when
 *     status is 0; both scores are 0 for a non-finite pose
 *   volume (n, 2T+1, 2R+1, 2R+1) int32: every S(k, a, b) at [k + T][a + R][b + R]
 * mask[e] == 0 leaves all of env e's outputs unwritten.
 * flags: FFMP_MATCH_GLOBAL — gather the map's bytes from global memory.  That is what the kernel does with or
 * without it: the other form, a copy in LDS of the box round the robot that holds every endpoint, gave the same
 * bits, was measured slower and is not kept; the flag is accepted and changes nothing.
 * FFMP_E_ARG, with a message and before any HIP call, for: what ffmp_world_map refuses of cfg, cells, n_beams,
 * range_max, ranges_stride, pose_stride, map_env_stride and the map's alignment; radius, n_turns, min_valid or
 * min_gain out of range; unknown flag bits; ranges, beams, pose, map or turns NULL; all three outputs NULL; a
 * misaligned output; an output whose bytes overlap the map's; n < 0 or too large for one launch.  n == 0:
 * nothing is launched.
 * ffmp_scan_match_check: the checks that need no pointer, no launch (the kernel's LDS is static, 27 KiB, whatever
 * the shape: its budget is checked when the library is compiled). */
#define FFMP_MATCH_GLOBAL 1
int ffmp_scan_match(const ffmp_cfg_t* cfg, int64_t n, const float* ranges, int64_t ranges_stride, int32_t n_beams,
                    const float* beams, const float* pose, int64_t pose_stride, const uint8_t* mask, const int8_t* map,
                    int64_t map_env_stride, int32_t cells, const float* turns, int32_t n_turns, int32_t radius, float range_max,
                    int32_t min_valid, int32_t min_gain, float* pose_out, int32_t* info, int32_t* volume, int32_t flags,
                    void* stream);
int ffmp_scan_match_check(const ffmp_cfg_t* cfg, int32_t n_beams, int32_t cells, int32_t radius, int32_t n_turns,
                          float range_max, int32_t min_valid, int32_t min_gain, int32_t flags);

/* Wide-prior and global relocalisation (an addition within ABI 9: no existing symbol, struct, value or limit
 * changes): ffmp_scan_match's winner over a window far larger than its own — radius = R in 0..1024 cells,
 * n_turns = T in 0..512 — found by a pruned two-level correlative search (Olson 2009; the branch and bound of
 * 2-D SLAM stacks) in place of the exhaustive one.  The scores are integer sums of int8 cells, so the bound
 * below is exact and the pruned search returns the same winner, bit for bit, as the exhaustive search under
 * ffmp_scan_match's tie order.  No reference counterpart [unpinned]; the SPEC below is the definition.  Six
 * launches on the caller's stream, capturable, read-only on the map.
 * ranges, ranges_stride, n_beams, beams, pose, pose_stride, mask, map, map_env_stride, cells = Wc, turns (the
 * caller's (2T + 1, 2) table), range_max, min_valid, min_gain, pose_out, info, stream: exactly ffmp_scan_match's.
 * block = B in {2, 4, 8, 16}; min_score: any int32; work, work_bytes: a DEVICE workspace of the caller's,
 * 16-byte aligned, at least n * ffmp_scan_relocalize_work(cells, radius, n_turns, block) bytes.
 * The fine score S(k, a, b), a, b in -R..R, k in -T..T, is ffmp_scan_match's, word for word: valid_l, bx/by,
 * ck/sk, fp/fq with rintf, on_l,k with this call's R, the int32 sum over the cells inside the plane, fp and fq
 * converted to int only where on_l,k holds.
 * New definitions:
 *   M'[p][q] = M[p][q] inside 0..Wc-1, else 0
 *   X[p][q] = max over 0 <= i, j < B of M'[p+i][q+j], for any integer p, q (0 where the window misses the plane)
 *   nb = (2R + B) / B (integer division);  a0(j) = -R + j*B
 *   block (k, A, Cc), A, Cc in 0..nb-1, holds the shifts a in a0(A)..min(a0(A)+B-1, R), and b likewise from Cc
 *   U(k, A, Cc) = sum over l with on_l,k of X[fp_l + a0(A)][fq_l + a0(Cc)], int32
 * U >= S for every shift of the block: each term of S is one of the cells X takes the maximum over, or 0 <= X
 * where the cell is off the plane.
 * Schedule (part of the SPEC: it defines info[7]):
 *   1. the seed is the block with the largest U; ties go to the smallest linear index ((k+T)*nb + A)*nb + Cc
 *   2. S1 = the largest S over the seed's shifts
 *   3. the refined set = every block with U >= S1
 *   4. the winner = the best shift over the refined set under ffmp_scan_match's total order: larger S, then
 *      smaller a*a + b*b, then smaller |k|, smaller k, smaller a, smaller b
 * This is the exhaustive winner:
 *   the exhaustive winner has S >= S1,
 *   its block has U >= S, so it is in the refined set,
 *   and the same holds for every candidate that ties with it.
 * Gate: ffmp_scan_match's — status 0 for a non-finite pose word, valid < min_valid, S_best - S(0,0,0) < min_gain,
 * or the winner (0, 0, 0) — plus one rule: status 0 if S_best < min_score.  INT32_MIN disables the rule.
 * Outputs, DEVICE memory, each written only when non-NULL (not all three NULL):
 *   pose_out (n, 4) float32 and info (n, 8) int32, 16-byte aligned: exactly ffmp_scan_match's, but info[7] = the
 *     size of the refined set
 *   bounds (n, 2T+1, nb, nb) int32, 4-byte aligned: every U(k, A, Cc) at [k + T][A][Cc]
 * There is no volume: most of it is never computed.  An env with a non-finite pose word has no beam on: both
 * scores are 0 and the status is 0.  mask[e] == 0 leaves all of env e's outputs unwritten.
 * flags: FFMP_RELOC_EXHAUSTIVE — the refined set is every block: the same pose_out and info[0..6], info[7] =
 * (2T+1)*nb*nb.
 * ffmp_scan_relocalize_work: the workspace bytes per env, a multiple of 16; a host function with no HIP call;
 * negative (FFMP_E_ARG, with a message) for cells, radius, n_turns or block out of range; it does not shrink
 * when radius or n_turns grows.  Per env the bytes hold, in this order: a 64-byte header {refined count, S1,
 * S(0,0,0), valid, the seed's index, the beams on over all rotations}; per rotation the largest (U, smallest index), 2T+1 uint64; the partial
 * winners of the refinement's workgroups; per rotation the number of beams on, 2T+1 int32; per rotation the on
 * beams' cell pairs (fp + R) << 16 | (fq + R), room for FFMP_MAX_BEAMS each; U, (2T+1)*nb*nb int32; the
 * refined blocks' indices, as many int32; X, one byte per cell of the plane extended by B - 1 to either side,
 * stored X[p mod B][q mod B][p div B][q div B].  Nothing in it outlives the call.
 * FFMP_E_ARG, with a message and before any HIP call, for: everything ffmp_scan_match refuses of the shared
 * arguments; radius, n_turns or block outside the limits above; all three outputs NULL; work NULL or work_bytes <
 * n * bytes per env; a misaligned bounds (4 bytes) or work (16 bytes); an output or the workspace whose bytes
 * overlap the map's; an output that overlaps the workspace.  n == 0: nothing is launched.
 * ffmp_scan_relocalize_check: the checks that need no pointer, no launch. */
#define FFMP_RELOC_EXHAUSTIVE 1
int ffmp_scan_relocalize(const ffmp_cfg_t* cfg, int64_t n, const float* ranges, int64_t ranges_stride, int32_t n_beams,
                         const float* beams, const float* pose, int64_t pose_stride, const uint8_t* mask, const int8_t* map,
                         int64_t map_env_stride, int32_t cells, const float* turns, int32_t n_turns, int32_t radius,
                         int32_t block, float range_max, int32_t min_valid, int32_t min_gain, int32_t min_score,
                         float* pose_out, int32_t* info, int32_t* bounds, void* work, int64_t work_bytes, int32_t flags,
                         void* stream);
int ffmp_scan_relocalize_check(const ffmp_cfg_t* cfg, int32_t n_beams, int32_t cells, int32_t radius, int32_t n_turns,
                               int32_t block, float range_max, int32_t min_valid, int32_t min_gain, int32_t flags);
int64_t ffmp_scan_relocalize_work(int32_t cells, int32_t radius, int32_t n_turns, int32_t block);

/* Motion flow estimated from the scan (an addition within ABI 9: no existing symbol, struct or value
 * changes): the sensor-side counterpart of the flow planes of cfg.flow.  Two scan frames `lag` updates
 * apart and the two poses give a per-cell velocity in the current ego axes, in the layout and units of
 * obs.flow.  As ffmp_scan_frames it has no reference counterpart (the BEV node is outside the
 * reference's repository) [unpinned]; the SPEC below is the definition.  Integer arithmetic apart from
 * the warp and one float multiply.
 * SPEC, per env.
 * Motion: (cr, sr, tx, ty), the restart rule and the per-cell (ru, rv, inside) are exactly
 * ffmp_scan_map's: float64 from eight float32 words, rounded to float32, then float32 left to right,
 * rintf.
 * Hit planes: a cell index outside 0..G-1 reads 0 in every plane.
 *   Hc[i][j]   = cur[i][j] == 255
 *   Hp[i][j]   = inside && prev[(int)ru + G/2][(int)rv + G/2] == 255
 *   D(X)[i][j] = OR of X over the 3 x 3 neighbourhood of (i, j)
 * Restart: if the env restarts (first[e] != 0 or a non-finite motion value), every cell gets kind 0
 * and flow 0.
 * Cell with !Hc[i][j]: kind 0, flow 0.
 * Cell with Hc[i][j]: the block is a, b in -B..B.
 *   1. nc = sum Hc[i+a][j+b].  If nc < min_hits: kind 0.
 *   2. c0 = sum (Hc & !D(Hp))[i+a][j+b] + sum (Hp & !D(Hc))[i+a][j+b].  If c0 <= gate: kind 1,
 *      (du, dv) = (0, 0) — the cell is static within a cell of warp jitter.
 *   3. Otherwise search.  Visit the displacements |du|, |dv| <= R in ascending order of the key
 *      (du*du + dv*dv, du, dv).
 *        np_d = sum Hp[i+a-du][j+b-dv]
 *        cost = sum Hc[i+a][j+b] ^ Hp[i+a-du][j+b-dv]
 *      A displacement with np_d < min_hits is skipped.  The first displacement with a strictly smaller
 *      cost wins.  If none qualifies: kind 0.  Otherwise kind 2.
 * Flow:
 *   vx = (float)du * scale;  vy = (float)dv * scale
 * — one float32 multiply, converted to binary16 round-to-nearest-even under the compact format; the
 * value is 0.0 for kind 0 and kind 1.  The cell now at i was at i - du, so the sign is that of
 * obs.flow: world velocity in the current ego axes.  (A caller passes scale = res / (lag * dt).)
 * Mask: an env with mask[e] == 0 keeps all its cells of both outputs.
 * Known limits: one quantum is `scale`; a straight wall gives no motion along itself (the aperture
 * problem: the gate hides most of it); a disc that reflects off a wall between the two frames.
 * cfg: only grid and res are read.  cur / prev: DEVICE uint8 planes, env e at e * frame_env_stride
 * bytes, row i ego x, column j ego y — scan frames as ffmp_scan_frames writes them in FFMP_OBS_U8F16;
 * only == 255 (a hit) is looked at.  pose_now / pose_prev with their strides, mask, first: as in
 * ffmp_scan_map.  flow_out: (n, 2, G, G), env e at e * flow_env_stride elements, planes vx then vy;
 * format FFMP_OBS_F32: float32, FFMP_OBS_U8F16: binary16 (obs.flow under the compact layout).
 * kind_out: uint8 (n, G, G), env e at e * kind_env_stride bytes, or NULL.  Knobs: radius R 1..5,
 * block B 1..3, gate 0..98, min_hits 1..49.
 * FFMP_E_ARG, with a message and before any HIP call, for: a grid outside 8..512 or not a multiple of
 * 4; an unknown format; a knob out of range; scale not finite; cur, prev, pose_now, pose_prev or
 * flow_out NULL; a stride that is too small (frames and kinds G*G, flow 2*G*G, poses 4); misaligned
 * planes or strides (frames and kinds 4 bytes, float32 flow 16 bytes, binary16 flow 8 bytes, strides
 * multiples of 4 elements); overlapping flow_out and kind_out planes, or an output that overlaps the
 * frames; n < 0 or too large for one launch.  n == 0: nothing is launched.
 * ffmp_scan_flow_check: the checks that need no pointer (shape, format, knobs), no launch. */
int ffmp_scan_flow(const ffmp_cfg_t* cfg, int64_t n, const uint8_t* cur, const uint8_t* prev, int64_t frame_env_stride,
                   const float* pose_now, int64_t pose_now_stride, const float* pose_prev, int64_t pose_prev_stride,
                   const uint8_t* mask, const uint8_t* first, void* flow_out, int64_t flow_env_stride, uint8_t* kind_out,
                   int64_t kind_env_stride, int32_t format, float scale, int32_t radius, int32_t block, int32_t gate,
                   int32_t min_hits, void* stream);
int ffmp_scan_flow_check(const ffmp_cfg_t* cfg, int32_t format, float scale, int32_t radius, int32_t block, int32_t gate,
                         int32_t min_hits);

/* Predicted-occupancy frames (an addition within ABI 9: no existing symbol, struct or value changes):
 * the step that joins the flow planes (cfg.flow's, or ffmp_scan_flow's estimate) to ffmp_nav_field.  The
 * cells a moving obstacle is predicted to cover at about the time the robot could be there are marked
 * in a copy of the frame, and the navigation field planned over that copy passes behind a crossing
 * obstacle instead of steering for the gap it is about to fill.  No reference counterpart [unpinned]; the
 * SPEC below is the definition.
 * SPEC, per env.  F: the frame, G x G, row i ego x, column j ego y, c = G/2.  vx, vy: the flow planes,
 * m/s in the current ego axes, binary16 converted to float32 first.  Knobs: steps H 1..64; cps
 * (float32, cells per m/s per prediction step: a caller passes (float)(dt_pred / res)); pace 1..1024,
 * the chamfer units (5 per cell) the robot covers per prediction step; slack -1..255; bytes swept, other.
 *   occ[a]  = F[a] > 0                      (a NaN compares false)
 *   src[a]  = F[a] == 255
 *   su = vx[a] * cps;  sv = vy[a] * cps     (one float32 multiply each, no contraction)
 *   a source is skipped if su or sv is not finite, or both are 0
 *   for k = 1..H:
 *       ti = i + (int)rintf((float)k * su);  tj = j + (int)rintf((float)k * sv)     (half to even)
 *       skipped if (ti, tj) lies outside 0..G-1
 *       m = max(|ti-c|, |tj-c|);  n = min(|ti-c|, |tj-c|);  ka = (5*m + 2*n) / pace   (integer division)
 *       slack < 0  or  |k - ka| <= slack :  bit[ti][tj] = 1
 *   out[a]  = F[a] == 255 ? 255 : occ[a] ? other : bit[a] ? swept : 0                (uint8, whatever the inputs)
 *   n_swept = number of cells with bit && !occ
 * A rounded displacement of G cells or more (a product that overflows to infinity included) leaves
 * the grid from any cell: it is skipped and no integer is formed for it.
 * ka is the earliest prediction step at which the robot can stand on the cell: the chamfer 5-7
 * distance from the robot cell at `pace` units per step.  The gate: a cell is blocked only if an
 * obstacle is predicted there within `slack` steps of that moment, so a disc that will have passed
 * before the robot can arrive blocks nothing.  slack = -1 turns the gate off and blocks the whole
 * swept corridor.  Present occupancy always stays: cells a moving disc is about to vacate are not
 * freed (conservative on purpose).
 * Mask: an env with mask[e] == 0 keeps its cells of `out` and its n_swept.
 * Parity: integer arithmetic apart from the two multiplies and (float)k * s, and the bits are ORed, so
 * the order cannot matter: the kernel equals tests/flow_predict_ref.py bit for bit.
 * Known limits: the prediction is constant-velocity (no wall reflection, no robot-obstacle
 * interaction); a thin arc moving more than about two cells per step leaves one-cell gaps between
 * successive k (ffmp_nav_field's footprint dilation closes those); the robot's arrival time is a
 * straight-line bound that ignores the detour.
 * cfg: only grid is read.  frame: DEVICE (n, G, G), env e at e * frame_env_stride elements;
 * frame_format FFMP_OBS_F32: float32, FFMP_OBS_U8F16: uint8.  flow: DEVICE (n, 2, G, G), env e at
 * e * flow_env_stride elements, vy = vx + G*G; flow_format FFMP_OBS_F32: float32, FFMP_OBS_U8F16:
 * binary16 — the two formats are separate (uint8 scan frames beside float32 flow is a real
 * combination).  mask: (n) bytes or NULL.  out: DEVICE uint8 (n, G, G), env e at e * out_env_stride
 * bytes.  n_swept: DEVICE int32 (n) or NULL.  16-byte loads and stores are used where a plane's base
 * and env stride allow, 4-byte ones otherwise.
 * FFMP_E_ARG, with a message and before any HIP call, for: a grid outside 8..512 or not a multiple of
 * 4; an unknown format; a knob out of range; cps not finite or < 0; swept or other outside 0..255;
 * frame, flow or out NULL; a stride that is too small (frame and out G*G, flow 2*G*G); misaligned
 * planes or strides (bases 4 bytes, strides multiples of 4 elements); an out (or n_swept) that
 * overlaps an input; n < 0 or too large for one launch.  n == 0: nothing is launched.
 * ffmp_flow_predict_check: the checks that need no pointer (shape, formats, knobs), no launch. */
int ffmp_flow_predict(const ffmp_cfg_t* cfg, int64_t n, const void* frame, int64_t frame_env_stride, int32_t frame_format,
                      const void* flow, int64_t flow_env_stride, int32_t flow_format, const uint8_t* mask, uint8_t* out,
                      int64_t out_env_stride, int32_t* n_swept, int32_t steps, float cps, int32_t pace, int32_t slack,
                      int32_t swept, int32_t other, void* stream);
int ffmp_flow_predict_check(const ffmp_cfg_t* cfg, int32_t frame_format, int32_t flow_format, int32_t steps, float cps,
                            int32_t pace, int32_t slack, int32_t swept, int32_t other);

/* Potential field of any occupancy frame (an addition within ABI 9: no existing symbol, struct or value
 * changes): the clearance plane, the attractive + repulsive potential plane and its gradient at the robot
 * cell from a frame — state_m's, a visible, scan-built, accumulated or predicted one, or the caller's own —
 * instead of from the simulator's disc list, so that ffmp_policy_field can follow what a sensor shows.  No
 * reference counterpart [unpinned]; the SPEC below is the definition.
 * SPEC, per env.  F: the frame, G x G, row i ego x, column j ego y, c = G/2.  Knobs: occ_min 1..255, reach 1..32.
 *   obst[a] = F[a] >= occ_min               (a float compare for a float32 frame: a NaN is free)
 * Clearance, integer arithmetic:
 *   d2[a] = min of di*di + dj*dj over the obstacle cells b = a + (di, dj) inside the grid with
 *           |di| <= reach and |dj| <= reach;  65535 if there is none
 * The window is the square, not the disc: one obstacle at (20, 20) with reach 3 gives d2[23][23] = 18, and
 * 65535 at (24, 20).  An obstacle cell has d2 = 0.  A minimum is unique, so no order of evaluation shows.
 * Potential, float32, every expression left to right as written, no contraction, sqrt and the reciprocal
 * correctly rounded:
 *   ex = (float)i*res_f - half_f;  ey = (float)j*res_f - half_f
 *   gx, gy = goal_ego[e*goal_stride + 0..1]
 *   dx = ex - gx;  dy = ey - gy;  U = half_ka_f * (dx*dx + dy*dy)
 *   if d2 != 65535:
 *       d = sqrt((float)d2) * res_f;  d = fmaxf(d, rho_min_f)
 *       if d < rho0_f:  q = 1.0f/d - inv_rho0_f;  U = U + half_kr_f * (q*q)
 * The attractive term is the raster's; the repulsive term is Khatib's nearest-obstacle form over the cells of
 * the frame, deliberately NOT the sum over discs of obs.potential: the two planes differ wherever two
 * obstacles are within rho0 of a cell, and here the walls and anything else the frame holds repel too.  The
 * field is exact out to rho0 only if reach * res >= rho0; this entry point does not enforce that (reach is a
 * knob here; the Python surface enforces it).  A non-finite goal propagates as written: NaN planes and a NaN
 * gradient, to which ffmp_policy_field answers (0, 0).
 * potential_format: FFMP_OBS_F32 writes U, FFMP_OBS_U8F16 binary16, round to nearest even from the float32 U
 * as the compact raster converts.
 * Gradient, from the float32 U under either format, computed whether or not `potential` is given — the
 * expression of the env step, the layout ffmp_policy_field reads:
 *   grad[e] = ((U[c+1][c] - U[c-1][c]) * inv_2res_f, (U[c][c+1] - U[c][c-1]) * inv_2res_f)
 *   robot_d2[e] = d2[c][c], or -1 where that is 65535
 * Mask: an env with mask[e] == 0 keeps every output word.
 * Parity: the kernel equals tests/frame_potential_ref.py bit for bit (NaN payloads aside).
 * cfg: grid, res_f, half_f, half_ka_f, half_kr_f, rho0_f, inv_rho0_f, rho_min_f and inv_2res_f are read.
 * frame: DEVICE (n, G, G), env e at e * frame_env_stride elements — a strided view such as state_m[:, 1] of
 * the ring window passes; frame_format FFMP_OBS_F32: float32, FFMP_OBS_U8F16: uint8.  goal_ego: DEVICE
 * float32, env e at e * goal_stride (record words 8..9 with the record's stride, or an (n, 2) tensor).
 * mask: (n) bytes or NULL.  dist2: DEVICE uint16 (n, G, G) or NULL; potential: DEVICE (n, G, G) or NULL;
 * grad: DEVICE float32 (n, 2) or NULL; robot_d2: DEVICE int32 (n) or NULL.  Every pointer is 4-byte aligned;
 * env strides count elements, are multiples of 4 and >= G*G.  The frame is read with 16-byte loads where
 * its base and env stride allow; a lane stores the 4 cells it owns at once (16 bytes of float32, 8 of
 * binary16 or uint16) where the plane's base allows; 4-byte accesses otherwise.  With both planes NULL only
 * the rows the gradient needs are worked on.
 * FFMP_E_ARG, with a message and before any HIP call, for: a grid outside 8..512 or not a multiple of 4; an
 * unknown format; occ_min outside 1..255; reach outside 1..32; frame or goal_ego NULL; goal_stride < 2; all
 * four outputs NULL; a stride that is too small or misaligned, or a misaligned base; an output that overlaps
 * the frame or another output; n < 0 or too large for one launch.  n == 0: nothing is launched.
 * ffmp_frame_potential_check: the checks that need no pointer (shape, formats, knobs), no launch. */
int ffmp_frame_potential(const ffmp_cfg_t* cfg, int64_t n, const void* frame, int64_t frame_env_stride, int32_t frame_format,
                         const float* goal_ego, int64_t goal_stride, const uint8_t* mask, int32_t occ_min, int32_t reach,
                         uint16_t* dist2, int64_t dist2_env_stride, void* potential, int64_t potential_env_stride,
                         int32_t potential_format, float* grad, int32_t* robot_d2, void* stream);
int ffmp_frame_potential_check(const ffmp_cfg_t* cfg, int32_t frame_format, int32_t potential_format, int32_t occ_min,
                               int32_t reach);

/* The rollout (dynamic-window) planner (an addition within ABI 9: no existing symbol, struct or value changes):
 * A candidate commands (v, w), each rolled forward on the host through the robot's own unicycle into a table of
 * cell offsets, are tested step by step against the cost-to-go plane of ffmp_nav_field and against the cells the
 * moving obstacles cover AT THAT STEP — a cost per cell and time instead of ffmp_flow_predict's one gated plane —
 * and the admissible candidate that ends lowest on the field is chosen.  With the reference's 4 speeds x 7 turn
 * rates (robot/config.py:28-55) as the candidates, m = 7*vi + wi, the choice is also a valid action id.  No
 * reference counterpart [unpinned]; the SPEC below is the definition.
 * SPEC, per env.  c = G/2.  cost: an ffmp_nav_field cost plane, G x G uint16, 65535 = hard or unreachable.  F, vx,
 * vy: a frame and its flow planes exactly as ffmp_flow_predict takes them (binary16 converted to float32 first), or
 * both NULL: no moving sources.  Knobs: cps (float32, cells per m/s per rollout step: a caller passes
 * (float)(stride * dt / res)); src_reach R 0..G; A 1..64 candidates; H 1..32 steps.
 * traj: int16 (A, H + 1, 2), traj[m][k-1] the cell offset of candidate m from the robot cell after k steps,
 * traj[m][H] its probe (the endpoint pushed forward along the final heading); cmds: float64 (A, 2), the command
 * (v_m, w_m) of candidate m.  All trigonometry is the caller's; integers only from here on.
 * Moving sources (ffmp_flow_predict's rules):
 *   src[a]  = F[a] == 255, looked at only where |i - c| <= R and |j - c| <= R
 *   su = vx[a] * cps;  sv = vy[a] * cps     (one float32 multiply each, no contraction)
 *   a source is skipped if su or sv is not finite, or both are 0
 *   for k = 1..H:  t = a + ((int)rintf((float)k * su), (int)rintf((float)k * sv))     (half to even)
 *       skipped if t lies outside 0..G-1 or a rounded displacement is G cells or more (an overflow to
 *       infinity included: no integer is formed for it);  hit_k = the set of those t
 * Per candidate m:
 *   win(m)  = vel == NULL, or  fabs(v_m - vel[e][0]) <= dv_max && fabs(w_m - vel[e][1]) <= dw_max   (float64; a NaN fails)
 *   p_k     = c + traj[m][k-1]
 *   blocked at k:  p_k outside 0..G-1,  or  cost[p_k] == 65535,  or  p_k + f in hit_k for a footprint offset f of cfg
 *   kb(m)   = the first such k, H + 1 if there is none
 *   blocked_at[e][m] = win ? kb : 0          (uint8)
 *   admissible  iff  win && kb == H + 1
 * Score (uint32):  g = cost[p_H];  h = cost[c + traj[m][H]] if the probe lies in the grid on a cost below 65535,
 *   else 65534;  J = g + h.
 * Choice: the admissible m with the least J; the lowest m wins ties.
 * Outputs, each written only when non-NULL: choice int32 (n), -1 when no candidate is admissible; cmd float64
 * (n, 2), 16-byte aligned: cmds[choice], or (0, 0); score uint32 (n): J, or 0xFFFFFFFF; n_adm int32 (n), the
 * number of admissible candidates; blocked_at uint8 (n, A).
 * Mask: an env with mask[e] == 0 keeps every output word.
 * Parity: integer arithmetic apart from the two multiplies, (float)k * s and the float64 window test; the hits are
 * ORed and a minimum is taken, so no order shows: the kernel equals tests/dwa_ref.py bit for bit.
 * Limits.  |traj offset| <= 28 is the caller's contract (the table is device memory; config.rollout_table enforces
 * it): with |footprint offset| <= 3 everything a rollout can ask about lies within 31 cells of the robot — one
 * 64 x 64 window per step, one 64-bit word per window row.  An entry beyond 28 is still tested against the grid
 * and the cost plane, but not against the moving sources.  Known limits: present occupancy stays hard at every k
 * (the cost plane holds it: cells a disc is leaving are not freed); the prediction is constant-velocity; nothing
 * is checked between successive k (a thin obstacle faster than a cell per step can be stepped over); the
 * candidate set is discrete.
 * cfg: grid and the footprint offsets are read.  cost: DEVICE uint16 (n, G, G), env e at e * cost_env_stride
 * elements.  frame, frame_env_stride, frame_format, flow, flow_env_stride, flow_format: as for ffmp_flow_predict.
 * traj, cmds: DEVICE, shared by the envs.  vel: DEVICE float64 (n, 2), the robot's present (v, w), or NULL.
 * mask: (n) bytes or NULL.
 * FFMP_E_ARG, with a message and before any HIP call, for: a grid outside 8..512 or not a multiple of 4; an unknown
 * format; cps not finite or < 0; src_reach outside 0..G; A outside 1..64; H outside 1..32; dv_max or dw_max < 0 or
 * NaN; a footprint offset above 3 (max |footprint offset| + 28 > 31); cost, traj or cmds NULL; one of frame and
 * flow NULL without the other; every output NULL; a stride that is too small (cost and frame G*G, flow 2*G*G) or
 * so large that the n envs do not fit 64 bits of address;
 * misaligned planes or strides (cost 2 bytes; frame and flow 4 bytes with strides multiples of 4 elements; traj 4,
 * cmds and vel 8, choice, score and n_adm 4, cmd 16 bytes); an output that overlaps an input; n < 0 or too large
 * for one launch.  n == 0: nothing is launched.
 * ffmp_dwa_check: the checks that need no pointer (shape, formats, knobs, footprint), no launch. */
int ffmp_dwa(const ffmp_cfg_t* cfg, int64_t n, const uint16_t* cost, int64_t cost_env_stride, const void* frame,
             int64_t frame_env_stride, int32_t frame_format, const void* flow, int64_t flow_env_stride, int32_t flow_format,
             float cps, int32_t src_reach, const int16_t* traj, const double* cmds, int32_t A, int32_t H, const double* vel,
             double dv_max, double dw_max, const uint8_t* mask, int32_t* choice, double* cmd, uint32_t* score, int32_t* n_adm,
             uint8_t* blocked_at, void* stream);
int ffmp_dwa_check(const ffmp_cfg_t* cfg, int32_t frame_format, int32_t flow_format, float cps, int32_t src_reach, int32_t A,
                   int32_t H, double dv_max, double dw_max);

/* Standalone reward/done (FFMP.rewarder / rewarder2 semantics), n envs:
 *   scan:   (n, scan_len) float64 ranges (0 = skipped, as `if scan_data[i]`), or NULL
 *   local_map: float32 planes, env e at local_map + e*map_stride (G x G), or NULL
 *   collide_in: optional precomputed collision bytes (used when scan and map are NULL)
 *   goal_in: optional precomputed goal bytes (NULL: dist < goal_thr)
 *   rel_goal (n,2) float64, is_first (n) bytes, d0 (n) float64 in/out.
 * Outputs reward (n) float64, done / is_goal / collide (n) bytes. */
int ffmp_reward_done(const ffmp_cfg_t* cfg, int64_t n,
                     const double* scan, int32_t scan_len,
                     const float* local_map, int64_t map_stride,
                     const uint8_t* collide_in, const uint8_t* goal_in,
                     const double* rel_goal, const uint8_t* is_first, double* d0,
                     double* reward, uint8_t* done, uint8_t* is_goal, uint8_t* collide,
                     void* stream);

/* One call of the single-env surface — FFMP.rewarder / rewarder2 / reward_calculator / is_goal
 * (src/gym_ffmp/envs/ffmp.py:120-188; rewarder2 is the one env call src/train.py:577 makes per
 * step) — from one packed buffer: host_buf (pinned host memory, 16-byte aligned) -> dev_buf (device,
 * >= in_bytes) in one copy, one ffmp_reward_done launch (n = 1), the 24 output bytes back into
 * host_buf in one copy, then the stream is synchronized: the results are in host_buf on return.
 * Layout (bytes): outputs reward f64 @0, d0 f64 @8 (in: the episode-start distance, out: set on
 * is_first), done / is_goal / collide u8 @16, 17, 18; inputs rel_goal f64[2] @24, is_first /
 * collide_in / goal_in u8 @40, 41, 42, scan f64[scan_len] @48, the local map f32[map_grid^2] @map_off
 * (16-aligned, >= 48 + 8 scan_len).  flags: 1 = collide_in given, 2 = goal_in given, 4 = a local map
 * (cfg's footprint; cfg->grid need not equal map_grid), 8 = without a map and with at most
 * FFMP_PACKED_ARG_BEAMS beams, pass the inputs as kernel arguments and write the outputs straight
 * into host_buf through its device view (hipHostGetDevicePointer: pinned, mapped memory) — one
 * launch and a synchronize, no copies; host_buf not mapped: the copies as without the flag. */
#define FFMP_PACKED_ARG_BEAMS 360
int ffmp_reward_done_packed(const ffmp_cfg_t* cfg, void* host_buf, void* dev_buf, int64_t in_bytes, int32_t scan_len,
                            int64_t map_off, int32_t map_grid, int32_t flags, void* stream);

/* FFMP.is_collision: any local_map[(G/2+di), (G/2+dj)] > 0 over the footprint. */
int ffmp_footprint_collision(const ffmp_cfg_t* cfg, int64_t n, const float* local_map,
                             int64_t map_stride, uint8_t* collide, void* stream);

/* FFMP.is_collision2 over (n, L) ranges: collide = any(r != 0 && r < thr);
 * min_r = min over those beams (+inf if none), may be NULL. */
int ffmp_scan_collision(int64_t n, int32_t L, const float* ranges, double thr,
                        uint8_t* collide, float* min_r, void* stream);
int ffmp_scan_collision_f64(int64_t n, int32_t L, const double* ranges, double thr,
                            uint8_t* collide, double* min_r, void* stream);

/* Self-check of the raster's exact fast math (no reference counterpart: the potential plane is
 * [no reference]): which = 0 compares sqrt_rn with sqrtf, 1 compares rcp_rn with
 * 1.0f / d, over the float bit patterns [lo_bits, hi_bits).  Adds the mismatch count to
 * *mismatches and atomic-mins the first mismatching pattern into *first_bits (device memory). */
int ffmp_check_exact_math(int32_t which, uint32_t lo_bits, uint32_t hi_bits,
                          unsigned long long* mismatches, uint32_t* first_bits, void* stream);

/* The learner's dominant convolution on the matrix cores (the reference
 * Network's conv2, src/train.py:233-242 / 244-255 — nn.Conv2d(32, 64, kernel_size=32) — and any
 * stride-1, unpadded convolution with 32 or 64 channels in and out):
 *   y[b][p][n] = act(bias[n] + sum_{ky,kx,c} x[b][yp+ky][xp+kx][c] * w[ky][kx][n][c])
 * x NHWC bf16 [batch][h][wd][c]; w bf16 [kh][kw][n][c] (torch's [n][c][kh][kw] permuted); bias
 * fp32 [n] or NULL; `pad` zero cells on every side of x (0 <= pad < kh, kw);
 * kernel column kx reads input column xo + kx * dx (dx >= 1: 1 = the plain convolution);
 * y NHWC [batch][h+2pad-kh+1][wd+2pad-(kw-1)dx][n], fp32 or (FFMP_CONV_OUT_BF16) bf16; fp32
 * accumulation on v_mfma_f32_32x32x16_bf16 (products exact, sums in fp32).  x and w 16-byte
 * aligned.  With pad = k - 1 and the kernel flipped and transposed (w'[ky][kx][c][n] =
 * w[k-1-ky][k-1-kx][n][c]) it is the data gradient of the unpadded convolution.
 * FFMP_CONV_W_FRAG: w holds the same elements in the kernels' fragment order,
 * [kh][kw][n/32][c/16][2][32][8] — weight (ky, kx, output channel o, input channel i) at index
 * ((((ky*kw + kx)*(n/32) + o/32)*(c/16) + i/16)*2 + (i%16)/8)*256 + (o%32)*8 + i%8 — so that each
 * 64-lane weight fragment load reads 1 KiB contiguous (the small-image kernel of conv3 / conv4:
 * ~17 % faster); the results are bit-identical to the plain layout's.
 * FFMP_CONV_X_FOLD (pad 0, dx = F >= 2 dividing c into an even count c / F): x is the UNFOLDED
 * NHWC input [batch][h][wd+F-1][c/F] of a few-channel convolution whose F consecutive kernel
 * columns were folded into channels; the kernel reads the folded image x'[b][y][x][j*(c/F) + i] =
 * x[b][y][x+j][i] — c / F <= 16 channels, wd columns — from it directly (no materialized fold).
 * Returns FFMP_OK or a negative code (ffmp_last_error()). */
#define FFMP_CONV_RELU 1
#define FFMP_CONV_OUT_BF16 2
#define FFMP_CONV_W_FRAG 4
#define FFMP_CONV_X_FOLD 8
int ffmp_conv2d_fwd_bf16(const void* x, const void* w, const float* bias, void* y, int32_t batch, int32_t h,
                         int32_t wd, int32_t c, int32_t kh, int32_t kw, int32_t n, int32_t pad, int32_t dx,
                         int32_t flags, void* stream);

/* The weight gradient of the same convolutions (MFMA, bf16 operands, fp32 accumulation):
 *   part[k][ky][kx][n][c] = sum over the samples of chunk k and all output positions p of
 *                           g[b][p][n] * x[b][yp+ky][xp+kx*dx][c]
 * g NHWC bf16 [batch][h-kh+1][wd-(kw-1)dx][n] (the output gradient), x NHWC bf16
 * [batch][h][wd][c] (the forward input); part fp32 [chunks][kh][kw][n][c] (every element
 * written); the caller sums over the chunks (batch split into `chunks` consecutive ranges). */
int ffmp_conv2d_wgrad_bf16(const void* g, const void* x, float* part, int32_t batch, int32_t h, int32_t wd, int32_t c,
                           int32_t kh, int32_t kw, int32_t n, int32_t dx, int32_t chunks, void* stream);

/* The data gradient of the same convolutions with the batch as the GEMM's M (the backward of
 * src/train.py:235's conv2 through autograd, :426-428):
 *   dx[b][Y][X][n] = sum_{ky,kx,c} g[b][Y+ky-(kh-1)][X+kx-(kw-1)][c] * w[ky][kx][c/8][n][c%8]
 * (cells outside g are zero: the full convolution).  g NHWC bf16 [batch][hy][wy][c] (the output
 * gradient); w bf16 [kh][kw][c/8][n][8] = the flipped, transposed kernel w'[ky][kx][n][c] =
 * w[n'=c][c'=n][kh-1-ky][kw-1-kx] with its channels in 8-blocks ahead of n; dx NHWC
 * [batch][hy+kh-1][wy+kw-1][n], fp32 or (FFMP_CONV_OUT_BF16) bf16.  32 samples share each MFMA
 * block, so every issued product is a useful one.  c = 32 or 64, n = 32; output rows of <= 72
 * positions; two gradient rows of KQ = 2 k-steps in LDS (wy <= 40). */
int ffmp_conv2d_dgrad_bf16(const void* g, const void* w, void* dx, int32_t batch, int32_t hy, int32_t wy, int32_t c,
                           int32_t kh, int32_t kw, int32_t n, int32_t flags, void* stream);

/* Would ffmp_conv2d_fwd_bf16 (kind 0; with pad > 0 the data-gradient form),
 * ffmp_conv2d_wgrad_bf16 (kind 1; pad ignored) or ffmp_conv2d_dgrad_bf16 (kind 2: h, wd = the
 * gradient's hy, wy; pad, dx ignored) accept this shape?  Runs every check of the launch
 * (channels, batch <= 65535, 16 KiB input rows, the LDS ring / stage, wgrad rows of >= 8
 * positions) and launches nothing.  FFMP_OK, or FFMP_E_ARG with the reason in ffmp_last_error().
 * The learner asks before it routes a convolution to the matrix-core kernels, and keeps the
 * library convolution for shapes outside them (src/train.py:231-303 at any map size). */
int ffmp_conv2d_check(int32_t kind, int32_t batch, int32_t h, int32_t wd, int32_t c, int32_t kh, int32_t kw,
                      int32_t n, int32_t pad, int32_t dx);

/* Episode bookkeeping of the training loop, batched (one record per env, device memory).
 * Per env and per ffmp_episode_update, exactly as src/train.py:579-682 does per iteration:
 *   reach window  <- is_goal (last `window` flags, window <= 64; REACH_MEMORY_CAPACITY = 10)
 *   reach_rate    =  np.average(window)                                    (:587, float64)
 *   done          =  out.done || (max_steps > 0 && step == max_steps)      (:607)
 *   done:  episode += 1, step = 0, is_first = 1, and with FFMP_EP_ARMED (the reference's
 *          `brain.loss != None`, :620) and reach_rate > threshold: complete = 1 (sticky, :644)
 *   else:  step += 1, total_step += 1, is_first = 0                       (:681-682)
 * FFMP_EP_RESET_ITER: the reference loop spends one iteration observing each freshly reset world
 * (is_first: never at the goal, never colliding) before an action takes effect; a batched env
 * folds it into the step that resets.  With this flag that iteration is run here as well — in
 * init and right after each done — so the counters equal the reference loop's.
 * Kept on purpose: the window counts iterations (not episodes), and the iteration that ends an
 * episode does not count towards total_step. */
#define FFMP_EP_TOTALS 8  /* totals[]: env-steps (updates), episodes, goals, collisions,
                             truncations, completions, counted steps (total_step increments), 0 */
#define FFMP_EP_ARMED 1
#define FFMP_EP_RESET_ITER 2
typedef struct ffmp_episode {
  uint64_t* reach_bits; /* (N) bit k = is_goal k iterations ago (bit 0 newest) */
  int32_t* reach_len;   /* (N) flags in the window (<= window) */
  double* reach_rate;   /* (N) */
  int32_t* step;        /* (N) iterations in the current episode */
  int32_t* episode;     /* (N) episodes ended */
  int64_t* total_step;  /* (N) */
  uint8_t* is_first;    /* (N) 1 before the first iteration of an episode */
  uint8_t* complete;    /* (N) sticky completion flag */
  uint64_t* totals;     /* (FFMP_EP_TOTALS) running sums over all envs, or NULL */
} ffmp_episode_t;

/* Start the masked envs (mask NULL: all, and totals zeroed) from the loop's initial values
 * (:501-505: counters 0, empty window, is_first = 1, complete = 0), followed by the
 * reset-observation iteration when flags has FFMP_EP_RESET_ITER. */
int ffmp_episode_init(int64_t n, const uint8_t* mask, int32_t flags, ffmp_episode_t* ep, void* stream);
/* One env step for envs [0,n) from its flags (out.done, out.is_goal, out.collide,
 * out.truncated; reward unused).  max_steps = 0 when out.done already includes truncation. */
int ffmp_episode_update(int64_t n, const ffmp_out_t* out, int32_t window, int32_t max_steps,
                        double threshold, int32_t flags, ffmp_episode_t* ep, void* stream);

/* make_temporal_maps (src/train.py:474-486) over k frames of the mono BEV image — the code path
 * of the reference's INPUT_CHANNELS = k with one image channel: map_memory keeps the last k
 * frames and is refilled with the first frame of an episode (is_first).  Served from a frame
 * window (the seamless ring keeps W >= k frames in place):
 *   out[e][c] = frame of lag d = k-1-c of env e (c = 0 oldest, k-1 newest), with the lag clamped
 *               to min(d, since[e]) — since = steps since the env's reset (ffmp_state_t.t), or
 *               NULL for no clamp;
 *   the frame of lag d of env e is at frames + lag_offset[d] + e * env_stride (elements;
 *   lag_offset a HOST array of k entries).
 * elem_bytes 1 (uint8 frames), 2 or 4 (float32); plane = G*G elements; out (n, k, G, G)
 * contiguous.  frames, out, plane * elem_bytes, env_stride * elem_bytes and every lag offset in
 * bytes must be 16-byte aligned.  A pure copy: k planes read and k written per env. */
#define FFMP_MAX_SERIES 16
int ffmp_temporal_maps(int64_t n, const void* frames, const int64_t* lag_offset, int32_t k, int64_t env_stride,
                       int64_t plane, int32_t elem_bytes, const int32_t* since, void* out, void* stream);

/* The 4-channel BEV image [occupancy, R, G, B] of the reference's 12-channel option
 * (src/train.py:66 "INPUT_CHANNELS = 12 #[channel] = (occupancy(MONO) + flow(RGB)) * series(3
 * steps)", src/gym_ffmp/envs/ffmp.py:16): the series of 3 such images is ffmp_temporal_maps over a
 * ring of them (plane = 4*G*G).  occ: the newest frame of env e at occ + e * occ_env_stride
 * (state_m's newest plane); flow: the (n, 2, plane) motion-flow planes of cfg.flow (ego vx, vy);
 * out: channel c of env e at out + e * out_env_stride + c * plane.  compact 0: float32 occ / flow /
 * out, compact 1 (FFMP_OBS_U8F16): uint8 occ and out, binary16 flow.  The reference's RGB flow
 * image came from BEV nodes outside its repository; the encoding here (float32, in this order):
 *   R = clamp(rint(127.5 + 127.5 * (vx / vmax)), 0, 255), G = the same of vy,
 *   B = clamp(rint(255 * (sqrt(vx*vx + vy*vy) / vmax)), 0, 255)   (rint: half to even)
 * — zero velocity is (128, 128, 0); vmax = the obstacle speed bound (FFMPConfig.obst_vmax). */
int ffmp_bev_image(int64_t n, int32_t compact, const void* occ, int64_t occ_env_stride, const void* flow,
                   int64_t plane, float vmax, void* out, int64_t out_env_stride, void* stream);

/* Seamless frame ring — an optional allocation helper (the step / raster entry points above
 * still never allocate).  The temporal stack of make_temporal_maps (src/train.py:474-486)
 * keeps the previous frame beside the new one; kept in place as a ring of `slots` frame
 * planes, the [older, newest] pair is the view of two consecutive slots [p, p+1].  A plain
 * array has no slot after the last one, so such a ring must wrap (and rewrite both frames)
 * every slots-1 steps.  This ring reserves (slots + 1) * slot_stride bytes of virtual address
 * space over `slots` physical slots of `device` (HIP virtual memory management) and maps
 * virtual slot `slots` onto the physical pages of slot 0 a second time, so the pair [p, p+1]
 * exists for every p in [0, slots): the view slides by one slot per step forever.
 *   Slots are built from physical pieces (1 GiB for slots of >= 2 GiB, else one per slot);
 *   slot_stride = slot_bytes rounded up to a whole number of pieces (out).
 *   partner (optional, device pointer, partner_bytes): the plane the raster writes in lockstep
 *   with every slot (the potential plane).  Two lockstep store streams run ~25 % slower when
 *   their physical pages pair badly, so each piece position gets a piece measured (two-stream
 *   store probe, which overwrites the partner's bytes) to pair well with the partner bytes the
 *   raster writes beside it: the same offset when partner_bytes < 1.5 x slot_bytes (float32
 *   frames beside a float32 plane), twice the offset otherwise (uint8 frames beside a binary16
 *   plane, FFMP_OBS_U8F16).  NULL: no pairing.  The library remembers the best probe per partner
 *   ADDRESS (the pairing reference, see ffmp_ring_pair_forget): a caller that passes a partner
 *   MUST call ffmp_ring_pair_forget(device, partner) when it frees that plane, or a plane
 *   allocated later at the same address inherits the old plane's reference (ffmp_ring_pool_trim
 *   does not forget them since ABI 8).
 *   *base = the first virtual slot (device pointer); contents undefined.
 * Returns 0, FFMP_E_ARG, or FFMP_E_HIP (no VMM support, out of memory, ...; then use a plain
 * ring — ffmp_last_error() says which call failed).
 * ffmp_ring_destroy drops the creator's reference.  Nothing is ever unmapped while the process
 * runs (ROCm 7 can resolve a reused, re-mapped VMM address to the old allocation — see
 * ffmp_kernels.hip): once a ring's last reference is gone its pieces return to a process-wide
 * pool that later rings draw from (or whose memory ffmp_ring_pool_trim gives back, keeping the
 * addresses reserved).  ffmp_ring_pool_bytes: pooled bytes (device < 0: all).
 * ffmp_ring_info: out[0..4] = pieces, fresh pieces allocated, pairing probes, min and max
 * probe GB/s of the chosen pieces (0 without a partner); with cap >= 6 also out[5] = the partner
 * byte ratio fixed at create (1: float32 frames beside a float32 plane, 2: uint8 frames beside a
 * binary16 plane; a rebuild keeps it).  Returns the number of values written (5 or 6). */
typedef struct ffmp_ring ffmp_ring_t;
int ffmp_ring_create(int32_t device, int64_t slot_bytes, int32_t slots, const void* partner,
                     int64_t partner_bytes, ffmp_ring_t** ring, void** base, int64_t* slot_stride);
/* A new ring (new addresses) with the pieces of `old`'s slots in replace_mask (bit i = slot i)
 * replaced by other pieces (chosen as in ffmp_ring_create, never the replaced ones), the other
 * slots' pieces shared with `old`.  For a caller whose timing shows a slot pairing badly.
 * `old` stays valid: the caller can time both rings and destroy the slower one (the kept
 * slots are the same memory in both, so only one of them should be written from then on).
 * A piece returns to the pool when the last ring holding it is gone; the pool is drawn from
 * only after a device synchronize (ffmp_ring_create / rebuild), so GPU work still writing a
 * dropped ring never overlaps the piece's next use. */
int ffmp_ring_rebuild(ffmp_ring_t* old, uint64_t replace_mask, const void* partner, int64_t partner_bytes,
                      ffmp_ring_t** ring, void** base, int64_t* slot_stride);
int ffmp_ring_destroy(ffmp_ring_t* ring);
int ffmp_ring_info(const ffmp_ring_t* ring, double* out, int32_t cap);
int64_t ffmp_ring_pool_bytes(int32_t device);
/* Bytes of virtual address space the ring helper has reserved on `device` in this process (piece
 * home mappings + every ring's (slots + 1) virtual slots).  Reservations are never freed while the
 * process lives (the re-map hazard above), so this only grows: a process that builds and drops rings
 * in a loop runs out of GPU virtual address space after roughly (device VA) / (per-ring delta)
 * rebuilds (INTEGRATION.md §5 states the bound measured for C3).  FFMP_E_ARG for device < 0 or >= 64. */
int64_t ffmp_ring_va_reserved(int32_t device);
/* Give back the physical memory of pooled pieces of `device` beyond the first keep_bytes
 * (0: all of them): after a device synchronize (pieces of rings dropped while kernels may still
 * write them are drained first), every mapping of such a piece — its home mapping and the slots
 * of the dead rings that held it — is unmapped and its handle released.  The address ranges
 * stay reserved until exit, so no later mapping is ever placed at an address that once held
 * another allocation (the stale-resolution hazard above).  Rings still alive are untouched, and
 * so are the pairing references (see ffmp_ring_pair_forget).  *released (optional) = bytes given
 * back.  Returns 0, FFMP_E_ARG or FFMP_E_HIP.  (FFMPVec calls it after construction and on close,
 * keeping FFMPVec.pool_keep_bytes: an instance's unchosen pairing candidates and the pieces of
 * rings it dropped go back to the device.)  Replaces no reference interface: the reference keeps
 * its 2-frame stack as a host NumPy array (src/train.py:474-486). */
int ffmp_ring_pool_trim(int32_t device, int64_t keep_bytes, int64_t* released);
/* The pairing references — the best two-stream probe seen per (device, partner plane), the
 * early-accept bar of ffmp_ring_create / ffmp_ring_rebuild — are keyed by the partner plane's
 * address.  The owner of a partner plane forgets its references when it frees the plane (a plane
 * allocated later at the same address must not inherit them): ffmp_ring_pair_forget(device,
 * partner), partner NULL = every reference of the device.  Returns the number forgotten (>= 0) or
 * FFMP_E_ARG.  ffmp_ring_pair_refs: how many the device holds. */
int ffmp_ring_pair_forget(int32_t device, const void* partner);
int ffmp_ring_pair_refs(int32_t device);
/* A dlpack.h (v0.8) DLManagedTensor* of `bits` elements (8: uint8, 16/32/64: float) over `data` (element strides,
 * ndim <= 8), for consumers that take DLPack (torch.utils.dlpack.from_dlpack, CuPy, JAX).
 * Its deleter frees it and, when `owner` is a ring, drops the reference it took on it: a ring
 * is parked once ffmp_ring_destroy was called AND every such tensor was deleted.
 * NULL on bad arguments. */
void* ffmp_dlpack(void* data, int32_t device_type, int32_t device_id, int32_t ndim, const int64_t* shape,
                  const int64_t* strides, int32_t bits, ffmp_ring_t* owner);

#ifdef __cplusplus
}
#endif
#endif /* FFMP_H */
