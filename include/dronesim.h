/*
 * dronesim.h -- C ABI of the MI355X-native batched drone_env hot path.
 *
 * The reference (AndreuMatoses/scalable-collision-avoidance-RL) is pure Python
 * and has no FFI layer; its boundary for this path is the duck-typed surface of
 * class `drones` (drone_env.py:53-401).  Each entry point below replaces one
 * reference method, batched over E independent environments, and is what a
 * Python `ctypes` binding of that class loads (see INTEGRATION.md and
 * scalable_collision_avoidance_rl_amd/_native.py).
 *
 * Conventions
 *  - Every buffer is CALLER-OWNED DEVICE memory (hipMalloc / a torch tensor's
 *    data_ptr()), contiguous, env-major:
 *        pos, vel, act      float32 [E][N][2]
 *        reward, true_reward float32 [E][N]
 *        z                  float32 [E][N][k+1][c]   (c = 2 or 5)
 *        nbr_idx            int32   [E][N][k+1]      slot 0 = i, then the real
 *                                                    neighbours by ascending d_ij,
 *                                                    unused slots = -1
 *        n_coll             int32   [E]   ordered colliding pairs (always even)
 *        done               uint8   [E]
 *        t                  int32   [E]   internal_t of every env
 *  - The library allocates nothing persistent, never synchronises the host and
 *    enqueues all work on `stream` (a hipStream_t passed as void*; NULL = the
 *    null stream).  Pass the stream the neighbouring kernels run on.
 *  - Return value: 0 on success, a negative DRONESIM_E* code otherwise; nothing
 *    is thrown across the ABI.  dronesim_last_error() gives a thread-local
 *    description of the last failure.
 *  - Re-entrant; the only mutable state is that thread-local string and a per-device record of which kernels
 *    have been opted into > 48 KiB of dynamic LDS (hipFuncSetAttribute; guarded by a mutex).
 *  - One process drives one GPU; multi-GPU runs shard the E axis across
 *    processes (env_base keeps random streams independent of the sharding).
 */
#ifndef DRONESIM_H
#define DRONESIM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DRONESIM_VERSION 600           /* 0.6.0: dronesim_reset_observe (env.reset() as one launch); 0.5.0: the float64 verification entry
                                          points moved to libdronesim_verify.so (dronesim_verify.h), DroneMlpBf16.wscale */
#define DRONESIM_MAX_K 8               /* k_closest supported by the kernels */
#define DRONESIM_MAX_AGENTS 1024       /* one workgroup holds one env */
#define DRONESIM_MAX_OBSTACLES 1024    /* static discs of an obstacle list (12 KB staged per workgroup) */
#define DRONESIM_MAX_SENSE 4           /* obstacle list slots per agent */

#define DRONESIM_OK 0
#define DRONESIM_EINVAL (-1)           /* null pointer / size out of range */
#define DRONESIM_EUNSUPPORTED (-2)     /* k or N beyond the compiled kernels */
#define DRONESIM_ELAUNCH (-3)          /* HIP launch error (see last_error) */

/* Constants of one `drones` object (shared by all E envs).
 * Scalars: drone_env.py:27-30 (dim, dt, max_time_steps), :72 (collision_weight),
 * :269-270 (q = 2*dt, b = collision_weight*dt), :251 (done radius 0.2), :386 (1.1).
 * Arrays (device pointers): goal ring xF and safety distance d_hat from
 * generate_formation (:115-153), deltas after the clip of :85-89, radii (:75). */
typedef struct DroneParams {
    int32_t N;              /* n_agents, 2..DRONESIM_MAX_AGENTS                     */
    int32_t k;              /* k_closest, 1..min(N-1, DRONESIM_MAX_K)               */
    int32_t c;              /* columns of a z row: 2 (simplify_zstate) or 5         */
    int32_t max_steps;      /* max_time_steps (200)                                 */
    float dt;               /* 0.05                                                 */
    float q;                /* formation weight, 2*dt                               */
    float b;                /* collision weight, collision_weight*dt                */
    float done_radius;      /* 0.2                                                  */
    float ghost_factor;     /* 1.1                                                  */
    /* host-known bounds of the arrays below (the library never reads device
       memory on the host): used to pick the kernel variant and the early-out
       radius; when min == max for all three, the kernels take the constants from
       here instead of reading the arrays.  0 < d_hat_min <= d_hat_max required.    */
    float d_hat_min;
    float d_hat_max;
    float delta_min;
    float delta_max;
    float radius_min;
    float radius_max;
    const float *xF;        /* [N][2] */
    const float *d_hat;     /* [N]    */
    const float *delta;     /* [N]    */
    const float *radius;    /* [N]    */
    /* optional (NULL = zeros): the part of the float64 goal ring that float32 drops, xF_lo = (float)(xF64 - (double)xF),
       [N][2].  The kernels form x - xF as (x - xF) - xF_lo: the first difference is exact near the goal, so the offset,
       the arrival test (:251) and the ghost direction (:383-386) keep float32 RELATIVE accuracy there instead of an
       absolute ulp32(G) -- without it a ghost row of an agent 0.04 from its goal is 2e-5 off the reference's at G = 31. */
    const float *xF_lo;
} DroneParams;

/* drones.step(actions)                                   drone_env.py:214-258
 * Integrates pos += dt*act, vel = act IN PLACE, then evaluates rewards(),
 * distance_data() and localized_states() on the new state (:260-401), the
 * termination test (:247-254) and t += 1 (:256).                                  */
int dronesim_step(const DroneParams *p, float *pos, float *vel, int32_t *t, const float *act,
                  float *reward, float *true_reward, float *z, int32_t *nbr_idx,
                  int32_t *n_coll, uint8_t *done, int E, void *stream);

/* drones.rewards(state, ...) without integration         drone_env.py:260-293
 * (what init_agents runs to produce the first z_states / Ni, :208-210).
 * reward, true_reward, n_coll may be NULL (not written).  mask NULL = every env,
 * otherwise only envs with mask[e] != 0 are evaluated and written.                */
int dronesim_observe(const DroneParams *p, const float *pos, const float *vel,
                     float *reward, float *true_reward, float *z, int32_t *nbr_idx,
                     int32_t *n_coll, const uint8_t *mask, int E, void *stream);

/* drones.reset() / init_agents(): state part             drone_env.py:98-102, 171-205
 * Draws N distinct nodes of the div_x x div_y lattice (node (a,b) -> (a*pitch,
 * b*pitch), pitch = 2*1.1*l) per env with a counter-based Philox4x32-10 stream
 * keyed by (seed, env_base + e, episode[e], agent, round); zeroes vel and t and
 * increments episode[e] (int32 [E], device, in/out: how many times env e has been
 * reset -- kept on the device so that a captured hipGraph replays fresh streams).
 * mask as above.  node_out (int32 [E][N], node = a*div_y + b) may be NULL.
 * Follow with dronesim_observe() to refresh z / nbr_idx (:208-210).               */
int dronesim_reset(const DroneParams *p, int div_x, int div_y, float pitch,
                   uint64_t seed, int64_t env_base, const uint8_t *mask,
                   float *pos, float *vel, int32_t *t, int32_t *episode, int32_t *node_out,
                   int E, void *stream);

/* T consecutive drones.step() calls in ONE launch (the `while not finished` loop
 * of train_problem.py:82-107 with the actions known up front, e.g. RandomAgent,
 * SAC_agents.py:9-22).  act is [T][E][N][2]; every per-step output of
 * dronesim_step is written for every step into [T][...] buffers laid out as T
 * consecutive copies of the per-step layout; pos/vel/t hold the final state.
 * Envs are NOT reset inside the rollout (t keeps counting, done stays set).
 * For N = 64 the far filter's verdicts (taken with radius reach + skin, skin = 0.4 reach) are kept in
 * registers and reused until some agent of the env has moved more than skin/2: bit-identical results. */
int dronesim_rollout(const DroneParams *p, float *pos, float *vel, int32_t *t, const float *act,
                     float *reward, float *true_reward, float *z, int32_t *nbr_idx,
                     int32_t *n_coll, uint8_t *done, int E, int T, void *stream);

/* ---- episode bookkeeping on the device (round 2) -------------------------------------------------------
 * The rollout loop logs, per episode, the sums it accumulates on EVERY step (train_problem.py:72-74, 98-100,
 * 118-121):  total_episode_reward += mean(rewards), total_true_episode_reward += mean(true_rewards),
 * total_episode_collisions += n_collisions, t_iter += 1.  DroneEpisodeAcc is that record, one per env, kept in
 * device memory and updated by the step kernel itself (the per-env reward sums are one fixed-order wave reduction
 * in the kernel's epilogue: bit-reproducible, no extra launch, 48 B of traffic per env-step).
 *   ep_*    the episode in progress.  ep_return / ep_true_return hold sum_t sum_i r_i: DIVIDE BY N for the
 *           reference's figure (it adds the mean over agents each step).
 *   done_*  totals over the episodes this env has completed; `episodes` counts them.  An episode is retired
 *           (ep_* added into done_*, ep_* cleared) when the env is reset: by the step kernel itself under
 *           auto_reset, or by dronesim_reset_ex.
 * The caller zero-initialises the records once.  dronesim_episode_reduce sums them over the envs of a rank (fixed
 * order); multi-GPU runs all-gather that 8-double vector -- the path's only exchange.                         */
typedef struct DroneEpisodeAcc {
    double ep_return;           /* sum over steps of sum_i reward_i            train_problem.py:98  */
    double ep_true_return;      /* same for true_reward                         :99                  */
    int32_t ep_collisions;      /* sum of n_collisions                          :100                 */
    int32_t ep_len;             /* steps of the episode in progress (t_iter)    :110                 */
    int32_t episodes;           /* completed episodes                                                */
    int32_t reserved;
    double done_return;         /* totals over completed episodes               :118-121             */
    double done_true_return;
    int64_t done_collisions;
    int64_t done_len;
} DroneEpisodeAcc;              /* 64 bytes, one cache line per env */

/* Episode control of the *_ex entry points.  acc may be NULL (no bookkeeping).  auto_reset != 0: an env whose
 * `done` fires (drone_env.py:251) is re-sampled (exactly as dronesim_reset would: same Philox stream, so the
 * fresh states do not depend on which of the two did it), its record retired, its t zeroed and its observation
 * recomputed INSIDE the same launch -- what train_problem.py:132 does after the `while not finished` loop.
 * reward / true_reward / n_coll / done of that step still describe the finished episode's last transition;
 * pos / vel / t / z / nbr_idx hold the new episode's first state and observation.
 * The lattice (div_x, div_y, pitch), seed, env_base and episode[] have the meaning they have in
 * dronesim_reset and are needed when auto_reset or in-kernel random actions are used.                        */
typedef struct DroneEpisodeCtl {
    DroneEpisodeAcc *acc;       /* [E] device records, or NULL                                       */
    int32_t auto_reset;
    int32_t div_x;              /* lattice of dronesim_reset: nodes per axis ...              */
    int32_t div_y;
    float pitch;                /* ... and node spacing                                          */
    uint64_t seed;
    int64_t env_base;
    int32_t *episode;           /* [E] device, resets seen per env (in/out)                          */
    /* Terminal observation under auto_reset (all three optional, NULL = not wanted).  The reference's step() returns
     * the z-states and state of the FINAL state of an episode (drone_env.py:258) and its loop stores them as `new_z` of
     * the last transition (utils.py:244-249) before it resets (train_problem.py:132).  With auto_reset the launch that
     * ends an episode overwrites z / nbr_idx / pos with the NEW episode's first observation; when these pointers are
     * given, the finished env's terminal rows are kept here instead of being lost: written ONLY for envs whose `done`
     * fired in this launch (rows of other envs are left untouched), same layouts as z / nbr_idx / pos.
     * SIZE: dronesim_step_ex writes rows [e][i]; the fused rollouts (dronesim_rollout_ex / _rollout_random) write
     * the rows of an env that finishes at step s at [s][e][i], exactly like their z output: there all three buffers
     * must hold T x E x N rows.  Passing [E]-sized buffers to a rollout of T > 1 steps is a caller error the library
     * cannot detect (plain pointers).                                                                           */
    float *z_final;             /* step: [E][N][k+1][c];  rollout: [T][E][N][k+1][c]                 */
    int32_t *nbr_final;         /* step: [E][N][k+1];     rollout: [T][E][N][k+1]                    */
    float *pos_final;           /* step: [E][N][2];       rollout: [T][E][N][2]                      */
} DroneEpisodeCtl;

/* dronesim_step / dronesim_rollout with episode bookkeeping and optional in-kernel auto-reset.  ctl == NULL
 * behaves exactly like the plain entry points.                                                               */
int dronesim_step_ex(const DroneParams *p, const DroneEpisodeCtl *ctl, float *pos, float *vel, int32_t *t,
                     const float *act, float *reward, float *true_reward, float *z, int32_t *nbr_idx,
                     int32_t *n_coll, uint8_t *done, int E, void *stream);
int dronesim_rollout_ex(const DroneParams *p, const DroneEpisodeCtl *ctl, float *pos, float *vel, int32_t *t,
                        const float *act, float *reward, float *true_reward, float *z, int32_t *nbr_idx,
                        int32_t *n_coll, uint8_t *done, int E, int T, void *stream);

/* dronesim_step_ex with its arguments marshalled ONCE: a rollout loop calls step() with the same buffers every time
 * (only the actions and, possibly, the stream change), and through an FFI that converts arguments one by one
 * (ctypes, cgo, JNI) the 14-argument form costs more host time than the launch.  The host class keeps one
 * DroneStepCall per (env, output binding) -- per storage slot when stepping into a RolloutStorage -- and makes a
 * 3-argument call per step (drone_env.py:214, train_problem.py:94).  Same checks, same launch, same result.   */
typedef struct DroneStepCall {
    const DroneParams *p;
    const DroneEpisodeCtl *ctl;         /* NULL = plain dronesim_step                                         */
    float *pos;
    float *vel;
    int32_t *t;
    float *reward;
    float *true_reward;
    float *z;
    int32_t *nbr_idx;
    int32_t *n_coll;
    uint8_t *done;
    int32_t E;
    int32_t reserved;
} DroneStepCall;
int dronesim_step_call(const DroneStepCall *call, const float *act, void *stream);

/* T fused steps whose actions are drawn INSIDE the kernel: RandomAgent.forward, SAC_agents.py:9-22
 * (clip(-1 + 2 rand(2), -1, 1)) for every agent and step, from the counter-based stream
 *   philox4x32-10(ctr = (agent, env_base + e, t[e] >> 1, episode[e]); key = (seed.lo ^ 0x52414E44, seed.hi)),
 *   words 2 (t & 1), 2 (t & 1) + 1 -> a = -1 + (w >> 8) * 2^-23   (uniform on the 2^24-point grid of [-1, 1))
 * keyed by the env's own step and episode counters: no action pool is read (44 B per agent-step instead of 52),
 * results do not depend on how the env axis is sharded or on T.  ctl is required (seed, env_base, episode; acc
 * and auto_reset optional).  act_out ([T][E][N][2], may be NULL) records the actions drawn.  Other buffers as
 * dronesim_rollout; any of reward / true_reward / n_coll may be NULL.                                         */
int dronesim_rollout_random(const DroneParams *p, const DroneEpisodeCtl *ctl, float *pos, float *vel, int32_t *t,
                            float *act_out, float *reward, float *true_reward, float *z, int32_t *nbr_idx,
                            int32_t *n_coll, uint8_t *done, int E, int T, void *stream);

/* T fused steps in CLOSED LOOP with a classical controller (control_test.py:30-45: proportional_control /
 * gradient_control feeding env.step): the action of step s is computed inside the launch from the positions the
 * env holds before step s -- exactly what dronesim_control(kind, u_max) returns on them -- so a step costs neither a
 * second launch nor a round trip of the actions through memory.
 *   kind    DRONESIM_CONTROL_PROPORTIONAL or DRONESIM_CONTROL_GRADIENT (anything else: DRONESIM_EINVAL)
 *   u_max   the controller's clip, > 0 (<= 0 or NaN: DRONESIM_EINVAL)
 * ctl may be NULL: a plain rollout without the episode layer.  With ctl->auto_reset an env that finishes at step s
 * is re-sampled inside the launch and its action at step s + 1 is the controller's on the NEW episode's positions.
 * act_out ([T][E][N][2], may be NULL) records the actions applied; replayed through dronesim_rollout_ex they give the
 * same outputs bit for bit, and results do not depend on how T is split into calls.  Other buffers as
 * dronesim_rollout_random; any of reward / true_reward / n_coll may be NULL.  c = 5 observations of envs whose rows
 * do not fit the LDS tile (n_agents x k_closest near the size limit) return DRONESIM_EUNSUPPORTED.             */
int dronesim_rollout_control(const DroneParams *p, const DroneEpisodeCtl *ctl, int kind, float u_max,
                             float *pos, float *vel, int32_t *t, float *act_out, float *reward, float *true_reward,
                             float *z, int32_t *nbr_idx, int32_t *n_coll, uint8_t *done, int E, int T, void *stream);

/* dronesim_reset that also retires the episode records of the envs it resets (those with ep_len > 0).        */
int dronesim_reset_ex(const DroneParams *p, const DroneEpisodeCtl *ctl, const uint8_t *mask,
                      float *pos, float *vel, int32_t *t, int32_t *node_out, int E, void *stream);

/* env.reset() as ONE launch (drone_env.py:98-102 -> init_agents :171-212 -> rewards :208): draws the lattice nodes exactly
 * as dronesim_reset does (same Philox stream, same acceptance rule: node ids bit-identical), writes pos / vel = 0 /
 * t = 0 / episode += 1, retires the episode records of the envs it resets when ctl->acc is set (as dronesim_reset_ex), and
 * computes the first observation z / nbr_idx of the new state like dronesim_observe -- from registers and LDS, without a
 * second launch or a round trip of the state through HBM.  ctl supplies div_x, div_y, pitch, seed, env_base, episode
 * (required) and acc (optional); mask as in dronesim_reset; node_out ([E][N], may be NULL) records the nodes drawn.      */
int dronesim_reset_observe(const DroneParams *p, const DroneEpisodeCtl *ctl, const uint8_t *mask,
                           float *pos, float *vel, int32_t *t, int32_t *node_out,
                           float *z, int32_t *nbr_idx, int E, void *stream);

/* out[0..7] = sums over the E records of (done_return, done_true_return, done_collisions, done_len, episodes,
 * ep_return, ep_true_return, ep_len), float64, one launch, fixed summation order (bit-reproducible).          */
#define DRONESIM_EPISODE_REDUCE_DOUBLES 8
int dronesim_episode_reduce(const DroneEpisodeAcc *acc, int E, double *out, void *stream);

/* Classical controllers, batched (deterministic action sources for rollouts and tests):
 *   kind DRONESIM_CONTROL_PROPORTIONAL  proportional_control(state, env)      drone_env.py:652-679
 *        u = k_gain (xF - x), norm capped at u_max (reference: k_gain = 1, u_max = 1)
 *   kind DRONESIM_CONTROL_GRADIENT      gradient_control(state, env, u_max)   drone_env.py:609-650
 *        u = clip(-(2 (x - xF) - 0.1 sum_{j != i, d_ij <= dhat_i} (x_i - x_j) / (d_ij |x_i - x_j|)), +-u_max)
 * pos [E][N][2] in, act [E][N][2] out.  Reads p->N, xF, xF_lo, d_hat, radius; with d_hat_max / radius_max set (> 0 / >= 0)
 * the gradient controller of envs of >= 40 agents finds its partners through the step kernel's cell-mask far filter.  */
#define DRONESIM_CONTROL_PROPORTIONAL 0
#define DRONESIM_CONTROL_GRADIENT 1
int dronesim_control(const DroneParams *p, int kind, const float *pos, float *act, float u_max,
                     int E, void *stream);

/* The statistic the rollout loop logs per step (train_problem.py:98-100, 118-120), accumulated on the device:
 *   acc[0] += sum reward, acc[1] += sum true_reward, acc[2] += sum n_coll, acc[3] += E N, acc[4] += E   (float64)
 * reward / true_reward [E][N], n_coll [E] as written by dronesim_step.  One launch, fixed summation order
 * (bit-reproducible).  scratch: DRONESIM_STATS_SCRATCH_DOUBLES doubles of device memory, zero-initialised once by
 * the caller and owned by one accumulator.  Multi-GPU runs all-gather `acc` (the path's only exchange).            */
#define DRONESIM_STATS_SCRATCH_DOUBLES 769
int dronesim_episode_stats(const float *reward, const float *true_reward, const int32_t *n_coll, int E, int N,
                           double *acc, double *scratch, void *stream);

/* Learner-side reductions over a stored rollout, buffers laid out [T][E][N] like the
 * outputs of dronesim_rollout / T calls of dronesim_step:
 *   dronesim_returns    Monte-Carlo return  G[t] = r[t] + gamma G[t+1],  G[T-1] = r[T-1]
 *                       (SAC_agents.py:304-307); `done` ([T][E] uint8, may be NULL) restarts the scan:
 *                       G[t] = r[t] where done[t] != 0.
 *   dronesim_advantage  weight of the actor loss  w[t,i] = gamma^t / N * sum_{j in Ni[t]} (G[t,j] - V[t,i])
 *                       (SAC_agents.py:333-351); nbr_idx [T][E][N][K1] is the neighbour list the action was
 *                       based on (slot 0 = i, -1 = empty); with `done` the exponent restarts after every
 *                       episode end.
 *   dronesim_neighbour_advantage   the PPO learner's advantage (SAC_agents.py:498-501, :512-513), no gamma^t, no 1 / N:
 *                       adv[t,i] = sum_{j in Ni[t]} G[t,j] - c V[t,i],  c = 1 (per_neighbour = 0: ONE baseline against the
 *                       neighbour sum, the reference's form) or c = |Ni[t]| (per_neighbour = 1).  G, V, adv [T][E][N],
 *                       nbr_idx as for dronesim_advantage; independent of `done` (nothing runs along t).  */
int dronesim_returns(const float *reward, const uint8_t *done, float gamma, float *G,
                     int T, int E, int N, void *stream);
/*   dronesim_lambda_returns   bootstrapped lambda-returns, TD(lambda) / GAE(gamma, lambda), for windows that cut episodes
 *                       (the reference trains on whole episodes and has no such function).  V [T+1][E][N]: V[t] the value of
 *                       the observation step t acted on, V[T] that of the observation after the last step.  Per column,
 *                       backwards from Gn = V[T]:
 *                         G[t] = r[t]                                                  where done[t] != 0 (terminal: no
 *                                                                                      bootstrap across an episode end)
 *                         G[t] = r[t] + gamma ((1 - lam) V[t+1] + lam Gn)              otherwise;        Gn = G[t]
 *                         A[t] = G[t] - V[t]                                           (GAE; G = A + V is the lambda-return)
 *                       reward, G, A [T][E][N]; `done` [T][E] uint8, may be NULL; G or A may be NULL, not both.  lam in
 *                       [0, 1]: 0 is the one-step TD target, 1 Monte-Carlo with a bootstrap at the window's end -- with
 *                       lam = 1 the columns of envs with done[T-1] != 0 are bit-identical to dronesim_returns.  EINVAL for a
 *                       NULL reward / V, both outputs NULL, T < 0, E < 0, N < 1, lam outside [0, 1], NaN lam or gamma;
 *                       T = 0 or E = 0 enqueues nothing.  One kernel launch (no memset nodes: graph-capturable).   */
int dronesim_lambda_returns(const float *reward, const uint8_t *done, const float *V, float gamma, float lam, float *G, float *A,
                            int T, int E, int N, void *stream);
/*   dronesim_episode_ends   the KIND of every episode end of a stored auto_reset window, recovered from the window itself.
 *                       `done` is "every agent within done_radius of its goal" OR "time limit" (drone_env.py:251), and the
 *                       terminal observation of every finished episode is in z_final [T][E][N][d] (d = (k+1) c floats per
 *                       agent, the first two of them the agent's own offset (zx, zy) from its goal).  With
 *                       outside(t,e,i) = !(sqrtf(fmaf(zy, zy, zx zx)) <= done_radius) -- the step kernel's own test; a
 *                       non-finite offset is outside --
 *                         ends[t][e] = 0   where done[t][e] == 0
 *                                      1   terminal: done, no agent outside (arrival, also on the last allowed step)
 *                                      2   truncated: done, some agent outside (this can only be the time limit)
 *                       The truncated ends of env e are ranked from the BACK of the window, k = number of truncated ends of e
 *                       at later t:  slot_t[k][e] = t ([M][E] int32, -1 where e has no k-th),  z_trunc[k][e] = z_final[t][e]
 *                       ([M][E][N][d], all zeros where slot_t is -1: every element is written by this call),  n_trunc[e] =
 *                       their count.  A truncated end with k >= M is demoted to ends = 1 (n_trunc > M tells); nothing is
 *                       read or written out of range.  EINVAL for a NULL argument, T < 0, E < 0, N < 1, d < 2, M < 1, a NaN
 *                       done_radius; E = 0 enqueues nothing.  Up to three kernel launches on `stream`, no host
 *                       synchronisation, no memset nodes, no atomics: graph-capturable and bit-identical run to run.
 *   dronesim_lambda_returns_ends   dronesim_lambda_returns with `ends` ([T][E] uint8 as above) in the place of `done`, and
 *                       Vend [M][E][N], the values of the terminal observations z_trunc.  Per column, backwards from
 *                       Gn = V[T] with a counter k = 0:
 *                         ends = 0            G[t] = r[t] + gamma ((1 - lam) V[t+1] + lam Gn)     (dronesim_lambda_returns' step)
 *                         ends = 1            G[t] = r[t]                                         (its done step)
 *                         ends = 2, k <  M    G[t] = r[t] + gamma Vend[k][e][i],  k += 1          (independent of lam: both terms
 *                                                                                                 of the mix are that value)
 *                         ends = 2, k >= M    G[t] = r[t]
 *                         A[t] = G[t] - V[t]
 *                       With ends in {0, 1} the outputs are bit-identical to dronesim_lambda_returns with done = ends; Vend is
 *                       read only at steps with ends = 2.  EINVAL as dronesim_lambda_returns, and for a NULL ends / Vend or
 *                       M < 1; T = 0 or E = 0 enqueues nothing.  One kernel launch.   */
int dronesim_episode_ends(const uint8_t *done, const float *z_final, int T, int E, int N, int d, float done_radius,
                          uint8_t *ends, int32_t *slot_t, int32_t *n_trunc, float *z_trunc, int M, void *stream);
int dronesim_lambda_returns_ends(const float *reward, const uint8_t *ends, const float *V, const float *Vend, int M, float gamma,
                                 float lam, float *G, float *A, int T, int E, int N, void *stream);
int dronesim_advantage(const float *G, const float *V, const int32_t *nbr_idx, const uint8_t *done,
                       float gamma, float *w, int T, int E, int N, int K1, void *stream);
int dronesim_neighbour_advantage(const float *G, const float *V, const int32_t *nbr_idx, int per_neighbour, float *adv,
                                 int T, int E, int N, int K1, void *stream);

/* Policy evaluation over a stored window (benchmark_agent.py:59-106, :148-156): the table of the FIRST episode of every
 * env.  reward, true_reward, V, G [T][E][N] float32, n_coll [T][E] int32, done [T][E] uint8 as the step launches write
 * them.  L_e = 1 + min{t : done[t][e] != 0}, 0 when no step of the window ended an episode.
 *   ep_len [E] int32                      L_e  (required)
 *   ep_collisions [E] int32               sum_{t < L} n_coll[t][e]  (needs n_coll)
 *   agent_return, agent_true_return [E][N] float64   sum_{t < L} of the float32 rewards, each widened to double first
 *   ep_return, ep_true_return [E] float64 (1 / N) sum_i agent_return[e][i], agents in ascending order (:85-86, :98-99: the
 *                                         sum over steps of mean(rewards)); each needs its agent_* array
 *   G [T][E][N] float32                   the WHOLE window's Monte-Carlo returns, bit-identical to dronesim_returns
 *   mean_adv [E][N] float64               (1 / L) sum_{t < L} ((double)G[t][e][i] - (double)V[t][e][i])  (:105; needs V)
 * Every output but ep_len may be NULL; V may be NULL (and is not read without mean_adv); n_coll may be NULL without
 * ep_collisions.  Envs with L_e = 0 get zeros everywhere except G.  Two launches on `stream` (the column scan, then one
 * thread per env); no float atomics: results are bit-identical run to run.                                            */
int dronesim_episode_eval(const float *reward, const float *true_reward, const int32_t *n_coll, const uint8_t *done,
                          const float *V, float gamma, int32_t *ep_len, int32_t *ep_collisions,
                          double *agent_return, double *agent_true_return, double *ep_return, double *ep_true_return,
                          float *G, double *mean_adv, int T, int E, int N, void *stream);

/* Per-episode safety tables of the same FIRST episode (L_e as above), from the stored post-step observations: z [T][E][N][k1 c]
 * float32 (row 0 of a record = x_i - xF_i, row 1 = x_j - x_i of the closest neighbour), nbr [T][E][N][k1] int32 (slot 1 = j, or
 * -1 for a ghost row), done [T][E] uint8; radius, delta [N] float32.  z_final / nbr_final (same shapes; both or neither): the
 * terminal observations of an auto_reset window -- the observation of step t is z_final[t] / nbr_final[t] where t = L - 1 and
 * they are given, z[t] / nbr[t] otherwise.  With |v| = sqrtf(fmaf(vy, vy, vx vx)) and j = nbr[t][e][i][1]:
 *   clearance(t,e,i) = min(|row 1| - radius[i] - radius[j], delta[i])  where 0 <= j < N,  delta[i] otherwise (a ghost row or
 *                      any id outside [0, N): radius is never indexed with it)
 *   min_clearance [E][N] float32     min_{t < L} clearance(t,e,i)
 *   goal_dist_final [E][N] float32   |row 0| of the observation of step L - 1
 *   arrive_step [E][N] int32         the smallest t + 1 <= L with |row 0| <= done_radius after step t, -1 if there is none
 *   ep_min_clearance [E] float32     min_i min_clearance[e][i], agents in ascending order  (needs min_clearance)
 *   ep_goal_dist_max [E] float32     max_i goal_dist_final[e][i], agents in ascending order  (needs goal_dist_final)
 *   ep_arrived [E] uint8             1 when no agent has !(goal_dist_final <= done_radius): dronesim_episode_ends' own test, a
 *                                    non-finite offset counts as outside -- equal to (ends[L-1][e] == 1)  (needs goal_dist_final)
 * min / max keep a NaN (numpy.minimum / maximum).  Envs with L_e = 0: NaN in the float tables (0 is a meaningful clearance),
 * arrive_step -1, ep_arrived 0.  Every output but ep_len may be NULL.  EINVAL for a NULL z / nbr / done / radius / delta /
 * ep_len, exactly one of z_final / nbr_final, T < 0, E < 0, N < 1, N > 1024, k1 < 2, c not in {2, 5}, a NaN done_radius, a
 * per-env output without the per-agent table it needs.  E = 0 enqueues nothing; T = 0 writes the L = 0 values.  Loads are as
 * wide as c, k1 and the alignment of z / z_final allow (16, 8 or 4 bytes), never misaligned.  Two launches on `stream` (the
 * column scan, then one thread per env and table); no atomics, no memset nodes: graph-capturable, bit-identical run to run. */
int dronesim_episode_safety(const float *z, const int32_t *nbr, const float *z_final, const int32_t *nbr_final, const uint8_t *done,
                            const float *radius, const float *delta, float done_radius, int T, int E, int N, int k1, int c,
                            int32_t *ep_len, float *min_clearance, float *goal_dist_final, int32_t *arrive_step,
                            float *ep_min_clearance, float *ep_goal_dist_max, uint8_t *ep_arrived, void *stream);

/* counts[min(v, n_bins)] += 1 for every e < E with values[e] = v >= 0 and (valid == NULL or valid[e] != 0): counts
 * [n_bins + 1] int64, the last bin takes the overflow (the collision histogram of benchmark_agent.py:148-156).
 * accumulate == 0: the kernel writes the counts itself (no memset); != 0: it adds to what is there.  One launch.    */
int dronesim_histogram_i32(const int32_t *values, const uint8_t *valid, int E, int n_bins, int64_t *counts,
                           int accumulate, void *stream);

/* Batched per-agent policy / critic forward: N independent 3-layer MLPs, one per agent,
 * evaluated on x[E][N][d_in] in one launch on the matrix cores in exact float32.
 *   DiscreteSoftmaxNN  utils.py:255-309   d_in -> 300 relu -> 300 relu -> n_actions softmax; sample_kind 1
 *                      draws the action index and returns the unit vector at angle 2 pi a / n_actions
 *   NormalActorNN      utils.py:55-117    d_in -> 400 relu -> (200 | 200) relu -> (tanh mu[2] | sigmoid var[2]):
 *                      pass the two heads concatenated as one 400-wide second layer and a block-diagonal
 *                      [400][4] output matrix; sample_kind 2 draws a ~ N(mu, sqrt(var))
 *   CriticNN           utils.py:14-53     d_in -> 200 relu -> 200 relu -> 1, out_kind 0
 * Weights are stacked per agent, "in x out" row-major: w1 [N][d_in][h1], b1 [N][h1], w2 [N][h1][h2],
 * b2 [N][h2], w3 [N][h2][nout], b3 [N][nout] (torch Linear stores [out][in]: transpose when importing).
 * out [E][N][nout] (post-activation, may be NULL), act [E][N][2] and act_idx [E][N] (may be NULL).
 * Random stream: row e, agent i draw the four words of
 *   philox4x32-10(ctr = (i, env_base + e, counter.lo + t[e], counter.hi + episode[e]); key = (seed.lo, seed.hi)),
 * every counter word modulo 2^32 on its own (no carry from counter.lo + t[e] into the high word); t / episode
 * (int32 [E], device, may be NULL = 0) are the env's own step and episode counters, so a captured hipGraph draws
 * fresh numbers on every replay.  Categorical: u = (word 0 >> 8) / 2^24, the pick is the first j with u < cdf_j
 * (nout - 1 if there is none).  Gaussian: component d takes words (2 d, 2 d + 1): u1 = ((w >> 8) + 1) / 2^24,
 * u2 = (w' >> 8) / 2^24, act_d = mu_d + sqrt(var_d) sqrt(-2 ln u1) cos(2 pi u2).  Pinned draw by draw by
 * tests/test_gpu_sampling.py against tests/sampling_ref.py.                                            */
typedef struct DroneMlp {
    int32_t N, d_in, h1, h2, nout;
    int32_t out_kind;       /* 0 identity, 1 softmax, 2 tanh(first half) + sigmoid(second half).  Accuracy contract of kinds 1 / 2
                             * and of the sampling (round 5 on): the activations use the hardware's 1-ulp exp2 / rcp / log2 / sqrt /
                             * sin / cos -- ABSOLUTE error <= 1e-6 per output (tanh as 1 - 2 / (e^2y + 1): no relative accuracy
                             * for |y| << 1), so sampled actions are reproducible run to run but not bit-comparable with a libm build */
    int32_t sample_kind;    /* 0 none, 1 categorical -> unit-circle action, 2 Gaussian          */
    int32_t w2_layout;      /* 0: w2 = [N][h1][h2] (the reference's layout transposed, like w1 / w3);
                             * 1: w2 = float32 matrix-core fragments [N][ceil(h2/32)][ceil(h1/16)][2][64][4] with
                             *    w2[a][c][s][q][l][j] = W2_a[16 s + 8 (l >> 5) + 4 q + j][32 c + (l & 31)], zero beyond
                             *    h1 / h2 -- packed once per weight update, read with 16-byte coalesced loads (the fast
                             *    path of rounds 3-5).  Same arithmetic, float32 throughout.
                             *    The packed array must be 16-byte aligned (EINVAL otherwise).
                             * 2: (0.6.0; d_in <= 14; what the host class BatchedMLP passes) w2 = ONE stream per agent holding
                             *    W1, b1, W2 and W3 in the consumption order of the row-tile kernel (a wave owns 32 env rows
                             *    and every output chunk; layers meet in registers): [N][B][4][64][4] float32 with
                             *    B = dronesim_mlp_rt_blocks(h1, h2, nout) blocks of four 1-KiB pieces [lane = 32 half + i][4]:
                             *      passes P = ceil(C2 / 7), chunks per pass = ceil(C2 / P), C1 = ceil(h1/32), C2 = ceil(h2/32);
                             *      per pass p (output chunks S_p): for c1 < C1: L1(c1), L2(c1, c2) for c2 in S_p; then -- nout > 4
                             *      only -- L3(c2) for c2 in S_p; behind the last pass 4 zero blocks;
                             *      L1(c1): piece 0 = W1[2 r + half][32 c1 + i], r = 0..3; piece 1 = the same for r = 4..6,
                             *              then b1[32 c1 + i] in lanes < 32; pieces 2, 3 zero;
                             *      L2(c1, c2): piece q = W2[32 c1 + 8 q + 4 half + j][32 c2 + i], j = 0..3;
                             *      L3(c2):     piece q = W3[32 c2 + 8 q + 4 half + j][i]       (zero beyond d_in / h1 / h2 / nout).
                             *    w1, b1 are not read (may be NULL); b2, b3 as always; w3 = the plain [N][h2][nout] array when
                             *    nout <= 4 (layer 3 then runs on the vector ALU and the stream holds no L3 blocks), not read
                             *    otherwise.  Same arithmetic (float32 fmaf chains) in a different summation order; 16-byte aligned. */
    const float *w1, *b1, *w2, *b2, *w3, *b3;
} DroneMlp;
int dronesim_mlp_rt_blocks(int h1, int h2, int nout);   /* blocks (4 KiB) per agent of the w2_layout = 2 stream              */
int dronesim_mlp_forward(const DroneMlp *m, const float *x, float *out, float *act, int32_t *act_idx,
                         uint64_t seed, uint64_t counter, int64_t env_base,
                         const int32_t *t, const int32_t *episode, int E, void *stream);

/* Opt-in bfloat16 variant of dronesim_mlp_forward (weights and activations in bf16, float32 accumulation,
 * ~16x the matrix rate; outputs agree with the float32 path to bf16 round-off, ~1e-2 relative).
 * Weights are pre-packed per matrix-core fragment: for a layer with K inputs and F outputs,
 *   wp[agent][c][s][lane][j] = W[kmap(s, lane >> 5, j)][32 c + (lane & 31)]   (0 beyond K or F)
 * for feature chunks c < ceil(F/32), k-steps s and j < 8, as bf16 (16 bytes per lane), with
 *   layers 1, 2:  kmap(s, h, j) = 16 s + 8 h + j
 *   layer 3:      kmap(s, h, j) = 16 s + 8 (j >> 2) + 4 h + (j & 3)   (the order in which a lane of the
 *                 layer-2 accumulator tile holds its features, so layer 3 is fed from registers).
 * k-steps: layer 1: 1 (d_in <= 16), layer 2: 2 ceil(h1/32), layer 3: 2 ceil(h2/32) with a single chunk
 * (nout <= 32).  */
typedef struct DroneMlpBf16 {
    int32_t N, d_in, h1, h2, nout, out_kind, sample_kind, reserved;
    const void *w1p, *w2p, *w3p;     /* packed bf16 fragments */
    const float *b1, *b2, *b3;       /* [N][h1], [N][h2], [N][nout] float32 */
    /* dronesim_mlp_forward_f16x2 only (NULL = all ones; ignored by the other entry points): [N][3] float32, POWERS OF TWO.
     * wscale[i][l] says that the packed image of layer l of agent i holds the weights MULTIPLIED by wscale[i][l] before
     * they were split; the kernel multiplies the layer's accumulators by 1 / wscale[i][l] (exact) before the bias-free
     * part meets the next layer.  A float16 part below 2^-14 is subnormal and keeps an ABSOLUTE 2^-24: an unscaled weight
     * of 0.05 is represented to 6e-7 of itself instead of 2^-22, which large activations multiply -- scaled so that the
     * layer's largest weight sits near 2^14, every weight keeps its 22 bits (round 5).  The factors live in DEVICE memory,
     * so the entry point cannot validate them: anything but a (normal) power of two makes the inverse inexact.
     * ABI NOTE: this field was appended in 0.5.0 -- a caller built against the 0.4.0 header passes a SHORTER struct and
     * must be rebuilt (dronesim_version() >= 500) before it calls dronesim_mlp_forward_f16x2.                         */
    const float *wscale;
} DroneMlpBf16;
int dronesim_mlp_forward_bf16(const DroneMlpBf16 *m, const float *x, float *out, float *act, int32_t *act_idx,
                              uint64_t seed, uint64_t counter, int64_t env_base,
                              const int32_t *t, const int32_t *episode, int E, void *stream);

/* float32-ACCURATE variant on the bf16 matrix instructions ("bf16x3"): every weight and activation is split by
 * truncation into three bf16 parts, v = hi + mid + lo exactly, and a product is the float32 sum of its six largest
 * partial products (hi*hi, hi*mid, mid*hi, hi*lo, lo*hi, mid*mid; the rest is below 2^-24 of the product).  Results
 * agree with dronesim_mlp_forward to float32 round-off (same 1e-5 bar against the reference's modules) at 6/16 of
 * its matrix time.  Same struct as the bf16 variant with a different weight image: w1p holds, per (agent, wave w < 4),
 * ONE stream of S = dronesim_mlp_bf16x3_stages(h1, h2) stages of 3 KiB -- a stage = the hi | mid | lo fragments
 * [3][64 lanes][8] bf16 of one (32-feature chunk, k-step), packed as for the bf16 variant with layers 2 AND 3 in the
 * "accumulator" k order (kmap(s, h, j) = 16 s + 8 (j >> 2) + 4 h + (j & 3)) and layer 1 in the linear one -- in the
 * order the kernel consumes them.  With W1(c) = layer 1, chunk c;  W2(c, ss, i) = layer 2, chunk w + 4 i, k-step
 * 2 c + ss;  W3(i, ss) = layer 3, k-step 2 (w + 4 i) + ss;  i running over the wave's chunks (w + 4 i < ceil(h2/32)):
 *     W1(0), W2(0,0,*), W1(1), W2(0,1,*), W2(1,0,*), W1(2), W2(1,1,*), ..., W2(C-1,1,*), W3(0,0), W3(0,1), W3(1,0), ...
 * then zero stages up to S.  [N][4][S][3][64][8] bf16 in all; w2p / w3p are unused, `reserved` must hold S.  */
int dronesim_mlp_bf16x3_stages(int h1, int h2);
int dronesim_mlp_forward_bf16x3(const DroneMlpBf16 *m, const float *x, float *out, float *act, int32_t *act_idx,
                                uint64_t seed, uint64_t counter, int64_t env_base,
                                const int32_t *t, const int32_t *episode, int E, void *stream);

/* The same with a two-part float16 split ("f16x2"): v = hi + lo with hi = float16(v), lo = float16(v - hi), exact to
 * 2^-22 of v (the float16 matrix instruction honours subnormal parts), and a product is the float32 sum of hi*hi,
 * hi*lo, lo*hi (the rest is below 2^-22 of the product): float32-level agreement with dronesim_mlp_forward (same 1e-5
 * bar) at 3/16 of its matrix time and 2/3 of the weight bytes of bf16x3.  DOMAIN: every (scaled, see
 * DroneMlpBf16.wscale) weight, input and hidden activation must be below 65504 in magnitude (float16 range) -- beyond
 * it the result is inf / NaN; use bf16x3 or dronesim_mlp_forward for such networks.  Weight image as for bf16x3 with two float16 parts per stage:
 * [N][4][S][2][64][8] float16, 2 KiB per stage.  */
int dronesim_mlp_forward_f16x2(const DroneMlpBf16 *m, const float *x, float *out, float *act, int32_t *act_idx,
                               uint64_t seed, uint64_t counter, int64_t env_base,
                               const int32_t *t, const int32_t *episode, int E, void *stream);

/* f16x2 with ROW-TILE ownership (0.6.0; d_in <= 16): a wave owns 32 env rows and every output chunk of layer 2, the four waves of a
 * workgroup share one weight ring; layer 3 runs in exact float32 on the vector ALU when nout <= 4 (the reference's Gaussian actor and
 * critic) and on the matrix cores, from the split of the relu'd layer-2 tiles, otherwise.  Same arithmetic contract as
 * dronesim_mlp_forward_f16x2 (two-part float16 split, three products, float32 accumulation).  DroneMlpBf16 fields as there, except:
 *   w1p      = ONE stream per agent, [N][B][4][64][8] float16 with B = dronesim_mlp_rt16_blocks(h1, h2, nout) blocks of four 1-KiB
 *              pieces ([lane = 32 half + i][8]), weights multiplied by wscale like the split image:
 *                passes P = ceil(C2 / 7), chunks per pass ceil(C2 / P); per pass p (output chunks S_p): for c1 < C1:
 *                  L1(c1)     = (W1 hi, W1 lo, 0, 0): piece[l][j] = part(W1[8 half + j][32 c1 + i])                (one 16-wide k-step)
 *                  L2(c1, c2) = (hi, lo of s = 2 c1), (hi, lo of s = 2 c1 + 1): piece[l][j] = part(W2[16 s + 8 (j >> 2) + 4 half + (j & 3)][32 c2 + i])
 *                for c2 in S_p; then, nout > 4 only, for c2 in S_p:
 *                  L3(c2)     = (hi, lo of s = 2 c2), (hi, lo of s = 2 c2 + 1): piece[l][j] = part(W3[16 s + 8 (j >> 2) + 4 half + (j & 3)][i])
 *                (outputs i >= nout zero); zero blocks up to B;
 *   w3p      = nout <= 4: the plain float32 [N][h2][nout] output layer (NOT multiplied by wscale; wscale[i][2] is not used);
 *              nout > 4: not read;
 *   reserved = dronesim_mlp_rt16_blocks(h1, h2, nout).                                                                       */
int dronesim_mlp_rt16_blocks(int h1, int h2, int nout);
int dronesim_mlp_forward_f16x2_rt(const DroneMlpBf16 *m, const float *x, float *out, float *act, int32_t *act_idx,
                                  uint64_t seed, uint64_t counter, int64_t env_base,
                                  const int32_t *t, const int32_t *episode, int E, void *stream);

/* Per-agent learner step of the batched MLPs (SAC_agents.py:280-357, SA2CAgents.train_NN), exact float32.  The DroneMlp must
 * describe the PLAIN weight arrays (w2_layout = 0, EINVAL otherwise): w1 [N][d_in][h1], b1 [N][h1], w2 [N][h1][h2], b2 [N][h2],
 * w3 [N][h2][nout], b3 [N][nout]; 1 <= d_in <= 64, h1, h2 <= 4096, nout <= 32; out_kind 0 with nout = 1, 1 with nout >= 2,
 * 2 with nout = 4 and an even h2 (the block-diagonal output layer of DroneMlp's NormalActorNN: w3[k][j] with
 * (k < h2/2) != (j < 2) is a structural zero -- its gradient is defined as 0, so it stays 0 under dronesim_adam_step).
 *
 * Flat gradient layout (grad, and Adam's m1 / m2): ONE buffer per network holding the six tensors in the order
 *   w1 | b1 | w2 | b2 | w3 | b3, each [N][...] like the weights: N * (d_in h1 + h1 + h1 h2 + h2 + h2 nout + nout) floats.
 *
 * dronesim_mlp_grad: gradients of the loss  sum_i L_i,  L_i = row_scale * sum_r l(r, i)  over R rows:
 *   x      float32 [R][N][d_in]   (a RolloutStorage window z_pre [T][E][N][d_in] is R = T E rows)
 *   out_kind 0 (critic):   l = (V_i(x_r) - target[r][i])^2                      target float32 [R][N]; row_scale = 1 / R is MSE
 *   out_kind 1 (softmax):  l = -weight[r][i] log softmax(o)[a]                   act float32 [R][N][2]: a = the index of the action list
 *                          entry (angle 2 pi a / nout) nearest to the stored unit action; weight float32 [R][N]
 *   out_kind 2 (Gaussian): l = -weight[r][i] sum_d [-0.5 log(2 pi var_d) - (act_d - mu_d)^2 / (2 var_d)],  mu = tanh, var = sigmoid
 * grad (flat, above) is OVERWRITTEN with dL_i / dparams_i, loss float32 [N] with L_i.  Rows go in chunks of rows_per_chunk (a
 * positive multiple of 64); ws is a device workspace of at least dronesim_mlp_grad_workspace(m, rows_per_chunk) bytes.  No float
 * atomics: the result is bit-identical run to run.
 *
 * dronesim_adam_step: per agent i, clip_grad_norm_ then torch.optim.Adam (no weight decay, no amsgrad), IN PLACE on the weight
 * arrays of m (the const pointers are written):
 *   grad_norm[i] = || grad_i ||_2 over the six tensors (pre-clip, float32 [N]);  grad_i *= min(1, max_norm / (grad_norm[i] + 1e-6))
 *   (the clipped gradient is written back);  step[i] += 1 (int32 [N], device memory: a captured graph advances it on every replay);
 *   m1 = m1 + (1 - beta1) (g - m1);  m2 = beta2 m2 + (1 - beta2) g^2;
 *   p -= lr / (1 - beta1^step) * m1 / (sqrt(m2) / sqrt(1 - beta2^step) + eps).
 * m1, m2: flat layout, zero before the first step.
 *
 * PPO with the clipped probability ratio (SAC_agents.py:410-573, SPPOAgents.train), actors only (out_kind 1 or 2; a critic is
 * EINVAL); same chunked chain, the same GEMM launches and the same log-probability expressions as dronesim_mlp_grad:
 * dronesim_mlp_logp: forward only.  logp[r][i] = log pi_i(act[r][i] | x_r)  (float32 [R][N], OVERWRITTEN): out_kind 1 the log
 *   softmax at the stored action's index, out_kind 2 the Gaussian log density with VARIANCE sigmoid (:558-573).  ws as for
 *   dronesim_mlp_grad (dronesim_mlp_grad_workspace bytes).  grad-free: no weight or gradient buffer is written.
 * dronesim_mlp_grad_ppo: gradients of  sum_i L_i,  L_i = -row_scale * sum_r min(r Adv, clamp(r, 1 - clip_eps, 1 + clip_eps) Adv)
 *   with  r = exp(logp - logp_old[r][i]),  Adv = adv[r][i]  (both float32 [R][N], constants of the loss; row_scale = 1 / R is
 *   the reference's mean).  As autograd gives it, a row contributes  -row_scale Adv r dlogp/dparams  unless the clipped branch
 *   is the strict minimum (Adv > 0 and r > 1 + clip_eps, or Adv < 0 and r < 1 - clip_eps), where it contributes 0.
 *   0 < clip_eps < 1.  grad (flat) and loss [N] are OVERWRITTEN as by dronesim_mlp_grad; so is stats, float32 [4][N]:
 *     stats[0][i] share of agent i's rows on the clipped branch, stats[1][i] mean of logp_old - logp (approximate KL),
 *     stats[2][i] / stats[3][i] min / max of r   -- per-row values reduced in a fixed order (no float atomics).
 *   ws: at least dronesim_mlp_grad_ppo_workspace(m, rows_per_chunk) bytes (the gradient workspace + 12 N rows_per_chunk).
 *   With the logp_old of dronesim_mlp_logp at the same weights and rows_per_chunk, logp == logp_old bit for bit: r is
 *   exactly 1, nothing is clipped and stats[1] is 0.                                                                     */
int dronesim_mlp_grad_workspace(const DroneMlp *m, int rows_per_chunk, size_t *bytes);
int dronesim_mlp_grad(const DroneMlp *m, const float *x, int R, float row_scale, const float *target, const float *act,
                      const float *weight, float *grad, float *loss, int rows_per_chunk, void *ws, size_t ws_bytes, void *stream);
int dronesim_mlp_grad_ppo_workspace(const DroneMlp *m, int rows_per_chunk, size_t *bytes);
int dronesim_mlp_logp(const DroneMlp *m, const float *x, int R, const float *act, float *logp, int rows_per_chunk, void *ws,
                      size_t ws_bytes, void *stream);
int dronesim_mlp_grad_ppo(const DroneMlp *m, const float *x, int R, float row_scale, const float *act, const float *logp_old,
                          const float *adv, float clip_eps, float *grad, float *loss, float *stats, int rows_per_chunk, void *ws,
                          size_t ws_bytes, void *stream);
int dronesim_adam_step(const DroneMlp *m, float *grad, float *m1, float *m2, int32_t *step, float lr, float beta1, float beta2,
                       float eps, float max_norm, float *grad_norm, void *stream);

/* Per-agent standardisation of a float32 [R][N] array with the agent on the fastest axis (the layout of a window's advantages
 * adv [T][E][N], R = T E); y == x (in place) is allowed.  Per agent i, with every float32 widened to float64 first:
 *   mean_i = (1/R) sum_r x[r][i],   std_i = sqrt((1/R) sum_r (x[r][i] - mean_i)^2)   (the population form),
 *   y[r][i] = (float)(((double)x[r][i] - mean_i) / (std_i + eps))   (formed as a product with the float64 reciprocal of
 *   std_i + eps: within 2^-52 of the quotient before the rounding to float; 0 where std_i + eps == 0).
 * stats, float32 [2][N] = (mean, std), is written by the kernels and may be NULL.  The second moment is taken about values of the
 * column itself, not as sum x^2 - R mean^2: a column at -500 +- 0.5 keeps its variance.  A column whose values are all equal
 * gives y = 0 exactly (no NaN, no inf); so does R = 1.
 * Deterministic: the rows are cut into slabs by a rule that depends on (R, N) only; one launch writes per-slab, per-agent
 * float64 partials into ws, a second folds them in a fixed ascending order and applies the map.  No float atomics, no memset
 * node, no host synchronisation: two calls on the same input give the same bits (in place or not, 16-byte aligned or not), and a
 * call inside a captured graph replays to the eager result.  ws: at least the bytes the workspace query returns for (R, N),
 * 8-byte aligned.
 * EINVAL: R < 1, N < 1, NULL x / y / ws, a short ws, eps < 0 (or NaN).                                                         */
int dronesim_standardize_workspace(int R, int N, size_t *bytes);
int dronesim_standardize(const float *x, float *y, float *stats, int R, int N, float eps, void *ws, size_t ws_bytes, void *stream);

/* The actor losses above with an entropy bonus, actors only (out_kind 1 or 2; a critic is EINVAL): the chunked chain of the
 * sibling entry point -- same GEMM launches, same workspace front part -- around a head that also carries the policy's entropy.
 * The loss of agent i becomes  L_i - ent_scale sum_r H_i(x_r)  (ent_scale = ent_coef / R: -ent_coef x the mean row entropy,
 * whatever row_scale the other term has); finite ent_scale >= 0.  Per row, in float32, with the expressions the heads form:
 *   out_kind 1:  lq_j = o_j - lse,  p_j = exp(lq_j),  H = -sum_j p_j lq_j;   dO_j += ent_scale p_j (lq_j + H)
 *                (H comes from lq, never from log(p): a saturated row has p_j = 0 and stays finite)
 *   out_kind 2:  H = sum_d 0.5 log(2 pi e var_d);   dO_{2+d} += -0.5 ent_scale (1 - var_d);   the mu outputs get nothing
 * In the PPO form the entropy's gradient is added on EVERY row, the rows on the clipped branch included.  loss [N] is the whole
 * objective (the sibling's term minus the entropy term).  entropy float32 [N] (PPO form: stats is float32 [5][N] and
 * stats[4][i] the entropy, stats[0..3] as above) is OVERWRITTEN with the MEAN row entropy of agent i, reduced from a per-row plane
 * in the fixed order of the loss.  ws: at least the bytes of the entry point's own workspace query (the sibling's workspace +
 * 4 N rows_per_chunk for the row entropies).  With ent_scale = 0 gradients, loss and stats[0..3] compare equal, element by
 * element, to the sibling's on the same inputs (an exact zero is added); the log-probability is the one dronesim_mlp_logp
 * computes, so with its logp_old the ratio is exactly 1 for any ent_scale.                                                      */
int dronesim_mlp_grad_ent_workspace(const DroneMlp *m, int rows_per_chunk, size_t *bytes);
int dronesim_mlp_grad_ent(const DroneMlp *m, const float *x, int R, float row_scale, const float *act, const float *weight,
                          float ent_scale, float *grad, float *loss, float *entropy, int rows_per_chunk, void *ws, size_t ws_bytes,
                          void *stream);
int dronesim_mlp_grad_ppo_ent_workspace(const DroneMlp *m, int rows_per_chunk, size_t *bytes);
int dronesim_mlp_grad_ppo_ent(const DroneMlp *m, const float *x, int R, float row_scale, const float *act, const float *logp_old,
                              const float *adv, float clip_eps, float ent_scale, float *grad, float *loss, float *stats,
                              int rows_per_chunk, void *ws, size_t ws_bytes, void *stream);

/* Two guards of the PPO learner's repeated steps on one window, both opt-in.  Same contract as the entry points above: kernels
 * only (no memset node), no allocation, no host synchronisation, no float atomics, bit-identical run to run, capturable in a
 * graph; an argument error returns DRONESIM_EINVAL before anything touches the device.  They run through the SAME chain, GEMM
 * and head kernels as their siblings, which take a nullable per-agent gate `active` (int32 [N], DEVICE memory; the older entry
 * points pass NULL): a workgroup, head row or per-agent sum whose agent has active[i] == 0 returns at entry.
 *
 * The per-agent KL early stop (actors only; the critic is never gated):
 * dronesim_mlp_grad_ppo_gated: dronesim_mlp_grad_ppo_ent plus `active` (NULL: nobody is gated), with stats float32 [6][N].
 *   stats[5][i] is the NON-NEGATIVE KL estimate of agent i, the mean over the rows of  k = expm1f(dl) - dl,  dl = logp - logp_old
 *   (the head's own dl): Schulman's (r - 1) - log r, formed without the cancellation of r - 1 (a k that rounds below 0 is 0).
 *   Per-row plane, reduced per agent in the fixed order of the other stats with float64 partial sums, carried in float64 across
 *   the chunks.  With the logp_old of dronesim_mlp_logp at the same weights it is exactly 0.  stats[1] (mean logp_old - logp)
 *   changes sign while a policy moves away and cannot be thresholded; this one can.
 *   With active == NULL or all ones, grad, loss and stats[0..4] compare equal element by element to dronesim_mlp_grad_ppo_ent's.
 *   For an agent with active[i] == 0 AT ENTRY no GEMM tile, head row or sum is computed, its slices of grad are left as they
 *   were, and loss[i] and stats[0..5][i] are written as NaN -- the NaN convention: a skipped step reports NaN, never a stale
 *   number.  The outputs of the active agents do not depend on which other agents are gated (bit for bit).
 *   ws: at least dronesim_mlp_grad_ppo_gated_workspace bytes (the sibling's + 4 N rows_per_chunk + 8 N), 8-byte aligned.
 * dronesim_kl_gate: one small kernel over active, taken (int32 [N], device memory).
 *   reset != 0 (kl may be NULL):  active[i] = 1, taken[i] = 0.
 *   otherwise: if active[i] and not (kl[i] <= target_kl): active[i] = 0   (NaN stops; equality continues; a stopped agent
 *   stays stopped until the next reset);  then, if active[i] is still set, taken[i] += 1.
 *   target_kl finite and > 0.  EINVAL: N < 1, NULL active / taken, NULL kl without reset, target_kl <= 0, NaN or inf.
 * dronesim_adam_step_gated: dronesim_adam_step plus `active` (not NULL).  An active agent gets exactly dronesim_adam_step's
 *   update, bit for bit; for a gated agent the weights, m1, m2, step[i] and its gradient slice are untouched and
 *   grad_norm[i] = NaN.
 * The learner's order per actor step is grad_ppo_gated -> kl_gate on that step's stats[5] -> adam_step_gated: the step on which
 * an agent crosses the threshold computes its gradient and discards it; every later step of the window skips the agent.
 *
 * PPO's clipped value loss (critics only, out_kind 0; an actor is EINVAL):
 * dronesim_mlp_grad_vclip: the critic chain of dronesim_mlp_grad with two more inputs, v_old float32 [R][N] (the values the
 *   window was collected with) and vf_clip (finite > 0, or +inf: never clamped).  Per row, with V = V_i(x_r), G = target:
 *     Vc = v_old + clamp(V - v_old, -vf_clip, +vf_clip)   (V itself where it is not clamped),   l = max((V - G)^2, (Vc - G)^2)
 *     dl/dV = 2 (V - G)  unless the clipped term is the STRICT maximum: there V is clamped and the gradient is 0.
 *   loss [N] is the clipped objective (times row_scale, summed); clip_fraction float32 [N] the share of zero-gradient rows, from
 *   one more per-row plane reduced in the fixed order.  Where no row is clamped, grad and loss equal dronesim_mlp_grad's bit
 *   for bit (the expressions are the same).  ws: at least dronesim_mlp_grad_vclip_workspace bytes (+ 4 N rows_per_chunk).    */
int dronesim_mlp_grad_ppo_gated_workspace(const DroneMlp *m, int rows_per_chunk, size_t *bytes);
int dronesim_mlp_grad_ppo_gated(const DroneMlp *m, const float *x, int R, float row_scale, const float *act, const float *logp_old,
                                const float *adv, float clip_eps, float ent_scale, const int32_t *active, float *grad, float *loss,
                                float *stats, int rows_per_chunk, void *ws, size_t ws_bytes, void *stream);
int dronesim_kl_gate(const float *kl, float target_kl, int32_t *active, int32_t *taken, int N, int reset, void *stream);
int dronesim_adam_step_gated(const DroneMlp *m, float *grad, float *m1, float *m2, int32_t *step, float lr, float beta1, float beta2,
                             float eps, float max_norm, float *grad_norm, const int32_t *active, void *stream);
int dronesim_mlp_grad_vclip_workspace(const DroneMlp *m, int rows_per_chunk, size_t *bytes);
int dronesim_mlp_grad_vclip(const DroneMlp *m, const float *x, int R, float row_scale, const float *target, const float *v_old,
                            float vf_clip, float *grad, float *loss, float *clip_fraction, int rows_per_chunk, void *ws,
                            size_t ws_bytes, void *stream);

/* Parameter sharing across agent groups (tied networks; csrc/learner.hip).  A sharing map ties the weights of the agents of a
 * group: they are bit-identical before and after every update.  It reaches the device in CSR form, two int32 arrays in DEVICE
 * memory that the caller builds once: group_ptr [n_groups + 1] and members [N]; the members of group g are
 * members[group_ptr[g] .. group_ptr[g + 1]), ascending, so the first is the group's LEADER (its lowest-numbered agent), and the
 * groups are ordered by leader.  Same contract as the entry points above: kernels only (no memset node), no allocation, no host
 * synchronisation, no atomics, bit-identical run to run, capturable in a graph.  EINVAL before any launch: a NULL pointer,
 * n_groups outside [1, N], and what the unshared sibling rejects.  The host cannot read the arrays without a synchronisation,
 * so every kernel skips a map entry outside [0, N): a bad map is never an out-of-bounds access.
 *
 * dronesim_adam_step_shared: dronesim_adam_step (active == NULL) or dronesim_adam_step_gated (active set) per GROUP:
 *   1. the group's gradient is the MEAN of its members' slices of grad, per element: float64 partial sums in ascending member
 *      order starting from the first member's value, divided by (double)|G|, rounded once to float32, written into the leader's
 *      slice of grad.  (The gradient of ONE network on the members' pooled rows with row scale 1 / (|G| rows): lr and max_norm
 *      keep their meaning.)
 *   2. the pre-clip norm, the clip and the Adam step of dronesim_adam_step on the LEADERS only, by the same kernels and hence
 *      the same instructions: the leader ends up bit for bit where dronesim_adam_step would put an agent holding that mean
 *      gradient.  Only the leader's slices of m1, m2 and grad are live -- after the call the leader's slice of grad holds the
 *      clipped group gradient; the other members' slices of the three buffers are left untouched.
 *   3. the leader's six weight tensors and its step counter are copied to every other member, and the group's pre-clip norm
 *      into every member's grad_norm[i].
 *   With active set a group's flag is its leader's: a stopped group changes nothing and all its members report NaN norms.
 *   A map of singletons is dronesim_adam_step(_gated) bit for bit.  Traffic per element of a group: 8 |G| + 44 bytes (each
 *   member's gradient read, each member's weight written, one 40-byte leader pass, one broadcast read) against 36 |G| unshared.
 * dronesim_kl_gate_shared: dronesim_kl_gate with one change -- the tested estimate of a group is the mean of its members' kl,
 *   float64 partial sums in ascending member order, compared in float64 -- and active / taken written identically for all
 *   members.  reset and the NaN rule are unchanged (a NaN member stops the group).
 * dronesim_mlp_tie: step 3 for the weights alone -- every member's six tensors become its leader's.                           */
int dronesim_adam_step_shared(const DroneMlp *m, float *grad, float *m1, float *m2, int32_t *step, float lr, float beta1,
                              float beta2, float eps, float max_norm, float *grad_norm, const int32_t *active /* or NULL */,
                              const int32_t *group_ptr, const int32_t *members, int n_groups, void *stream);
int dronesim_kl_gate_shared(const float *kl, float target_kl, int32_t *active, int32_t *taken, int N, int reset,
                            const int32_t *group_ptr, const int32_t *members, int n_groups, void *stream);
int dronesim_mlp_tie(const DroneMlp *m, const int32_t *group_ptr, const int32_t *members, int n_groups, void *stream);

/* Shuffled minibatches (csrc/minibatch.hip).  Both entry points only enqueue one kernel on `stream`: no memset node, no
 * allocation, no host synchronisation, no atomics; deterministic, and capturable in a graph.
 *
 * dronesim_row_permutation: perm (int32 [R], OVERWRITTEN) becomes a permutation of 0..R-1 that is a pure function of
 * (R, seed, *counter).  counter is a DEVICE pointer to one int32 that the kernel reads: with the counter in device memory (e.g.
 * the step counter dronesim_adam_step advances) a captured graph draws a fresh permutation on every replay.  One thread per row, no
 * sort.  The rule, in unsigned 32-bit arithmetic throughout -- a 4-round balanced Feistel network with cycle-walking:
 *   h = max(1, ceil(bitlen(R - 1) / 2)),  mask = 2^h - 1          (bitlen(0) = 0; R = 2^31 - 1 gives h = 16, the domain 2^32)
 *   a value v < 2^(2h) is split as  L = v >> h,  Rr = v & mask
 *   round k = 0..3:  (L, Rr) <- (Rr, L ^ (w0(Rr, k) & mask));  the network's result is (L << h) | Rr
 *   w0(a, k) = word 0 of Philox4x32-10 with counter (a, k, (uint32_t)*counter, 0) and key ((uint32_t)seed, (uint32_t)(seed >> 32))
 *   perm[r]: start from v = r and apply the network until the result is < R.
 * The network is a bijection of [0, 2^(2h)) and 2^(2h) < 4 R for R >= 2, so the walk is a bijection of [0, R) and a thread applies
 * the network fewer than 4 times on average.  1 <= R <= 2^31 - 1.  EINVAL: R < 1, NULL counter or perm.
 *
 * dronesim_gather_rows: ONE launch that gathers the rows of n_arrays (1..8) row-major arrays by perm (int32 [R], device memory,
 * entries in [0, R); an entry outside that range is skipped: its destination row is left as it was).  src, dst, row_bytes and
 * block_bytes are HOST arrays of n_arrays entries (read during the call, passed to the kernel by value); src[a] / dst[a] are
 * device addresses.  The R positions are cut into R / M blocks of M; for position p = b M + j (0 <= j < M) the row of array a is
 * copied from  src[a] + perm[p] row_bytes[a]  to  dst[a] + b block_bytes[a] + j row_bytes[a].  block_bytes[a] >= M row_bytes[a]: a
 * caller pads it (say to a multiple of 256) to start every block on an aligned address; the padding bytes are not written.
 * Rows are positive multiples of 4 bytes, at most DRONESIM_GATHER_MAX_ROW_BYTES, and need not be multiples of 16 (an array whose
 * row size, block size and two base addresses are all multiples of 16 moves in 16-byte pieces, any other in 4-byte pieces);
 * src[a], dst[a] and block_bytes[a] are multiples of 4.  The bytes are copied as they are: any element type.
 * src and dst arrays MUST NOT overlap each other (not checked: it cannot be checked cheaply); src[a] needs R rows, dst[a]
 * (R / M) block_bytes[a] bytes.
 * EINVAL: R < 1, M < 1, R % M != 0, n_arrays outside 1..8, a row size that is not a positive multiple of 4 (or above the limit),
 * block_bytes[a] < M row_bytes[a], a NULL pointer (perm, the four host arrays, any src[a] / dst[a]), an address or block size that
 * is not a multiple of 4.                                                                                                         */
#define DRONESIM_GATHER_MAX_ROW_BYTES (1 << 24)
int dronesim_row_permutation(int R, uint64_t seed, const int32_t *counter, int32_t *perm, void *stream);
int dronesim_gather_rows(const int32_t *perm, int R, int M, int n_arrays, const void *const *src, void *const *dst,
                         const int64_t *row_bytes, const int64_t *block_bytes, void *stream);

/* Observation normalisation (csrc/obsnorm.hip): running per-column statistics of float32 row matrices x [R][C], kept and applied
 * on the device.  C = N d_in columns, one per (agent, input column); a window z [T][E][N][d] or one step's observation
 * [E][N][k+1][c] is such a matrix without a copy.  state is float64 [3][C] = (count, mean, m2), table float64 [2][C] = (mean, inv),
 * both DEVICE memory that only the kernels read and write.  Kernels only: no memset node, no allocation, no host
 * synchronisation, no float atomics; one fixed reduction order that depends on (R, C) only -- the same bits run to run, for
 * 16-byte-aligned and merely 4-byte-aligned x, and inside a captured graph.
 *
 * dronesim_obsnorm_update: per column, over the FINITE values of x (NaN and +-inf are not counted), n_b, mean_b and M2_b, the sum
 *   of squared deviations from mean_b; every float32 is widened to float64 and shifted by a finite value of its column (or 0)
 *   before it is squared, so a column at -500 +- 0.5 keeps its variance.  Then Chan's rule, with d = mean_b - mean:
 *     n' = n + n_b,   mean' = mean + d n_b / n',   m2' = m2 + M2_b + d^2 n n_b / n'
 *   (a column with n_b = 0 keeps the bits of its state; count is a float64 holding an exact integer), and the table is rewritten:
 *     mean,  inv = 1 / sqrt(m2 / count + eps)   (0 where m2 / count + eps == 0);   count == 0:  mean = 0, inv = 1, the identity.
 *   An all-equal column has mean = the value and m2 = 0 exactly.  Two launches: per-slab partials into ws, then the fold, the
 *   merge and the table.  ws: at least dronesim_obsnorm_workspace(R, C) bytes, 8-byte aligned.
 *   EINVAL: R < 1, C < 1, NULL x / state / table / ws, eps < 0 (or NaN), a short or misaligned ws.
 * dronesim_obsnorm_apply: y[r][c] = (float)(((double)x[r][c] - mean_c) inv_c), then clamped to [-clip, clip] when clip is finite
 *   and > 0 (clip <= 0 or +inf: no clamp).  NaN in gives NaN out (the clamp is two comparisons, not fminf / fmaxf); +-inf gives
 *   +-clip, or +-inf without a clamp.  y == x (in place) is allowed.  16 bytes per lane where C % 4 == 0 and both pointers are
 *   16-byte aligned, else 4 bytes with the same lane-to-element map; a matrix of 32 MiB or more streams through non-temporal
 *   accesses.  EINVAL: R < 1, C < 1, NULL x / y / table.                                                                        */
int dronesim_obsnorm_workspace(int R, int C, size_t *bytes);
int dronesim_obsnorm_update(const float *x, int R, int C, double *state, double *table, double eps, void *ws, size_t ws_bytes,
                            void *stream);
int dronesim_obsnorm_apply(const float *x, float *y, int R, int C, const double *table, float clip, void *stream);

/* Reward normalisation (csrc/rewnorm.hip): return-based reward scaling over a stored window reward [T][E][N] with done [T][E],
 * kept and applied on the device.  NO mean is subtracted.  Every column (env e, agent i) carries a running discounted return
 * across windows in float64, ret [E][N] (the caller zeroes it once):
 *     R <- gamma R + r[t][e][i];   R is counted;   if done[t][e]: R <- 0 (after the count)
 * and the counted values go into per-group running moments state [3][n_groups] = (count, mean, m2), float64, m2 the sum of squared
 * deviations from the mean.  group [N] maps agent -> statistics group (ids in [0, n_groups), the CALLER validates them; NULL: one
 * group).  Only FINITE R are counted: a NaN or +-inf reward poisons its column's carry until that column's next done, those steps
 * are not counted, and the carry is NOT repaired.  Kernels only: no memset node, no allocation, no host synchronisation, no
 * float atomics; one fixed order that depends on (T, E, N, group) only -- the same bits run to run, for any alignment of
 * reward, and inside a captured graph.
 *
 * dronesim_rewnorm_update: three launches.  (1) a forward scan, one thread per column, consecutive threads on consecutive
 *   addresses at every t, staged by eight steps with the next stage requested before the current one is folded; per column the
 *   shifted float64 sums n, sum (R - K), sum (R - K)^2 (K: the column's first counted value; no division per step), converted once
 *   to (n, mean, M2) in ws -- 24 bytes per column against 4 T read.  (Un-pipelined -- request a stage, wait, fold -- the whole
 *   update took 93.3 us instead of 88 at T = 200 x 4096 envs x 64 agents and 79.7 instead of 73 at 200 x 512 x 256.)  (2) per agent, the envs in contiguous ascending runs and a
 *   fixed tree over the runs, Chan's rule.  (3) per group, its agents in ascending order; then Chan's rule into state, with
 *   d = mean_b - mean:  n' = n + n_b,  mean' = mean + d n_b / n',  m2' = m2 + M2_b + d^2 n n_b / n'  (a group with n_b = 0 keeps
 *   the bits of its state), and scale [N] is rewritten:
 *     scale[i] = 1 / sqrt(m2_g / count_g + eps),  g = group[i];   1 where count_g = 0;   1 where m2_g / count_g + eps == 0.
 *   The last rule differs from the observation table (inv = 0 there) on purpose: a zero scale would erase the reward signal.
 *   ws: at least dronesim_rewnorm_workspace(T, E, N) bytes, 8-byte aligned.
 *   EINVAL: T, E or N < 1, NULL reward / done / ret / state / scale / ws, gamma outside [0, 1] (or NaN), eps negative or not
 *   finite, n_groups outside [1, N], NULL group with n_groups != 1, a short or misaligned ws.
 * dronesim_rewnorm_apply: out[t][e][i] = (float)((double)reward[t][e][i] scale[i]), then clamped to [-clip, clip] when clip > 0
 *   (0: no clamp).  NaN stays NaN (the clamp is two comparisons).  out == reward (in place) is allowed.  16 bytes per lane where
 *   E N % 4 == 0 and both pointers are 16-byte aligned, else 4, with the same bits; a window of 32 MiB or more streams through
 *   non-temporal accesses.  EINVAL: T, E or N < 1, NULL reward / out / scale.                                                     */
int dronesim_rewnorm_workspace(int T, int E, int N, size_t *bytes);
int dronesim_rewnorm_update(const float *reward, const uint8_t *done, int T, int E, int N, double gamma, const int *group, int n_groups,
                            double *ret, double *state, double *scale, double eps, void *ws, size_t ws_bytes, void *stream);
int dronesim_rewnorm_apply(const float *reward, float *out, int T, int E, int N, const double *scale, float clip, void *stream);

/* Action shield: a local collision-avoidance filter between the policy and the step (csrc/shield.hip; DESIGN.md has the guarantee
 * and its conditions).  Per record (e, i): z [E][N][k1 c] float32 and nbr [E][N][k1] int32 are the observation the agent acts on
 * (row 0 = x_i - xF_i, rows 1..k = x_j - x_i of the k closest agents inside Delta, nbr[s] = j, an id outside [0, N) a ghost row),
 * act [E][N][2] the nominal action u, radius [N].  The half-planes a.x <= b, in this fixed order:
 *   1. the box: (+1,0), (-1,0), (0,+1), (0,-1), each with b = u_max (+inf: they never bind);
 *   2. for slot s = 1..k with j = nbr[s], p = floats 0, 1 of row s, d = |p|: skipped unless 0 <= j < N, j != i, d finite and
 *      d > 0; otherwise a = p / d, g = d - radius[i] - radius[j] - margin, b = rate max(g, 0) / dt.
 * act_out [E][N][2] = u*, the Euclidean projection of u onto the intersection (never empty: 0 satisfies every constraint);
 * intervened [E][N] uint8 and correction [E][N] float32 = |u* - u| may be NULL.  Where u satisfies every constraint as the kernel
 * evaluates it (float32: d = sqrt(fma(py, py, px px)), a = p (1 / d), g = ((d - radius[i]) - radius[j]) - margin,
 * b = (rate / dt) max(g, 0), violated where fma(ax, ux, ay uy) > b), act_out is u bit for bit, intervened 0, correction 0.  Where
 * a component of u is not finite, u is copied through, intervened 0, correction NaN.  act_out may alias act.  The correction
 * of a finite u is finite wherever |u* - u| is a float32 (the norm is taken of the components scaled by a power of two, so their
 * squares do not overflow for |u* - u| > 2^64).
 * One launch on `stream`, one thread per record, loads as wide as c, k1 and the alignment of z allow (16, 8 or 4 bytes), never
 * misaligned; no atomics, no workspace, no host synchronisation: graph-capturable, bit-identical run to run.  E = 0 enqueues
 * nothing.  EINVAL: NULL z / nbr / act / radius / act_out, E < 0, N outside 1..1024, k1 outside 2..DRONESIM_MAX_K + 1, c not in
 * {2, 5}, rate outside (0, 0.5], margin negative or not finite, u_max <= 0 or NaN, dt <= 0 or not finite.
 *
 * dronesim_shield_totals adds one call's planes to per-agent running totals (the caller zeroes them): interventions [N] int64
 * (intervened != 0), nonfinite [N] int64 (correction NaN), correction_sum [N] float64 and correction_max [N] float32 over the
 * corrections that are not NaN.  One launch, fixed reduction order (per lane the envs ascending with stride 256, one LDS tree, one
 * plain read-modify-write per agent), no float atomics: bit-identical run to run.  EINVAL: a NULL pointer, E < 0, N outside 1..1024. */
int dronesim_action_shield(const float *z, const int32_t *nbr, const float *act, const float *radius, float rate, float margin,
                           float u_max, float dt, int E, int N, int k1, int c, float *act_out, uint8_t *intervened,
                           float *correction, void *stream);
int dronesim_shield_totals(const uint8_t *intervened, const float *correction, int E, int N, int64_t *interventions,
                           int64_t *nonfinite, double *correction_sum, float *correction_max, void *stream);

/* Static obstacle discs (csrc/obstacles.hip, csrc/shield.hip; DESIGN.md has the guarantee and its conditions).  The step kernel,
 * never reads them: these entries work on stored observations, beside the step.
 *
 * Inputs: obstacles [M][3] float32 (x, y, r), one list shared by all envs, 0 <= M <= DRONESIM_MAX_OBSTACLES (may be NULL at
 * M = 0); xF [N][2] the goals; radius [N]; sense [N] the range of every agent.
 * Position, from the agent's OWN record (row 0 is x_i - xF_i; c = 2 or 5): x = fl32(z[0] + xF[i][0]), y = fl32(z[1] + xF[i][1]),
 * z[0], z[1] floats 0, 1 of row 0.
 * Gap to disc o: p = o.xy - (x, y), d = sqrtf(fmaf(p.y, p.y, p.x p.x)) (the correctly rounded square root),
 * gap = (d - radius[i]) - o.r.
 *
 * The sense entry, per record (e, i) of z [E][N][k1 c]: among the discs with gap <= sense[i] (a NaN gap is not in
 * range) the m smallest, 1 <= m <= DRONESIM_MAX_SENSE, ordered by gap ascending, then by id ascending.  Slot s of
 * orow [E][N][m][3] = (p.x, p.y, o.r), oid [E][N][m] = the id; empty slots (0, 0, 0) and -1.  Optional planes over ALL M discs, in
 * range or not: gap_min [E][N] (numpy.minimum: a NaN stays; +inf at M = 0) and hit [E][N] uint8 = gap_min <= 0.  One launch, one
 * thread per record, row 0 loaded 16, 8 or 4 bytes wide by the shield's alignment rule, the list staged once per workgroup in
 * LDS and read at wave-uniform addresses, the m best kept by sorted insertion in registers; no atomics, no workspace:
 * graph-capturable, bit-identical run to run.  E = 0 enqueues nothing.  EINVAL: NULL z / xF / radius / sense / orow / oid, E < 0,
 * N outside 1..1024, k1 outside 1..DRONESIM_MAX_K + 1, c not in {2, 5}, M outside 0..1024 (or NULL obstacles with M > 0), m
 * outside 1..4.
 *
 * The obstacle shield takes the half-planes of the plain shield entry unchanged and in their order (box, then neighbour
 * slots 1..k) and appends slot s = 0..m-1 of the record's list: skipped unless 0 <= oid < M and d = |row.xy| (as above, from the
 * stored p) is finite and > 0; otherwise a = row.xy / d, g = ((d - radius[i]) - row.r) - margin, b = (obstacle_rate / dt)
 * max(g, 0): at most 4 + 8 + 4 = 16 constraints, solved by the same incremental solve (one device function, instantiated for 12
 * and for 16 constraints).  obstacle_rate in (0, 1]: the disc does not move, so the agent may spend the whole budget.  Every
 * other argument, plane and property is the plain entry's; EINVAL also for NULL orow / oid, m outside 1..4, M outside 0..1024,
 * obstacle_rate outside (0, 1].  With every slot empty the output is the plain entry's bit for bit.
 *
 * The episode tables cover the FIRST episode of every env of a stored window z [T][E][N][k1 c], done [T][E], with L_e (ep_len)
 * exactly as the episode safety tables define it; the observation of step L - 1 comes from z_final where it is given (NULL: from
 * z).  With gap_min(t) the sense entry's plane at step t:  min_obstacle_gap [E][N] float32 = min over t < L of gap_min(t)
 * (a NaN stays);  obstacle_hit_steps [E][N] int32 = #{t < L : gap_min(t) <= 0};  ep_min_obstacle_gap [E] = the minimum over the
 * agents in ascending order;  ep_obstacle_hit_steps [E] int32 = the sum over the agents;  ep_len [E].  L_e = 0: NaN in the float
 * tables, 0 in the int tables.  Every table but ep_len may be NULL (a per-env table needs the per-agent one it reduces).  Two
 * launches on `stream` (one without per-env tables): the backward column scan with the disc loop in its step, then one thread
 * per (env, table); no atomics: graph-capturable, bit-identical run to run.  E = 0 enqueues nothing.  EINVAL: NULL z / done (with
 * T > 0) / xF / radius / ep_len, T or E < 0, N outside 1..1024, k1 < 1, c not in {2, 5}, M outside 0..1024 (or NULL obstacles with M > 0), a
 * per-env table without its per-agent one.
 *
 * Obstacle columns and obstacle cost -- what the networks and the reward see of the discs.  Both use the gap above, the ONE
 * float32 expression, so they agree with the sense entry bit for bit.
 * Columns: a record z[r][i] of d = k1 c floats becomes d + 3 m floats: floats [0, d) are the record's own bits, float
 * d + 3 s + (0, 1, 2) is slot s of the sense entry's list, (p.x, p.y, o.r), an empty slot (0, 0, 0) -- the range, the ordering (gap
 * ascending, then id ascending) and the NaN rule are the sense entry's own: the policy sees exactly the discs the shield constrains.
 * Cost: the reference's collision term (drone_env.py:268-334: b log(d_i / d_ij) over the Delta-neighbourhood, 9.99e3 for a
 * collision) with a disc in the neighbour's place.  Over ALL M discs in ascending id, accumulated in float32, with s = sense[i]:
 * 9.99e3 where gap <= 0;  logf(s / gap) where 0 < gap <= s (the correctly rounded quotient);  0 otherwise (a NaN gap, or s <= 0
 * with a positive gap, gives 0).  cost = fl32(weight sum); M = 0 gives 0.
 * The shaped reward of transition t is fl32(reward[t] - cost(observation after step t)): z_final[t] where done[t] and z_final is
 * given, the post-step observation z_post[t] otherwise.
 *
 * dronesim_obstacle_observe takes R rows of [N][k1 c] (a window ring of (T + 1) E rows, the truncated ends' M_t E rows or one
 * step's E rows pass without a copy) and writes x_out [R][N][k1 c + 3 m] and, where cost_out is not NULL, cost_out [R][N].  One
 * launch, one thread per record; the lists of a workgroup are parked in LDS and its 256 records leave as one contiguous run in
 * lane order (16-byte stores where x_out is 16-byte aligned, dword stores otherwise; the same bits either way).
 * dronesim_obstacle_reward is elementwise over (t, e, i) of z_post / z_final [T][E][N][k1 c], done [T][E], reward [T][E][N]: it
 * writes reward_out [T][E][N] (reward_out == reward, in place, is allowed) and, where not NULL, cost_out [T][E][N]; z_final may be
 * NULL.  One launch.  Both stage the list once per workgroup in LDS; no atomics, no workspace, no host synchronisation:
 * graph-capturable, bit-identical run to run.  R = 0 / T E = 0 enqueues nothing.  EINVAL: a NULL pointer other than obstacles at
 * M = 0, z_final and cost_out; R, T or E < 0, N outside 1..1024, k1 outside 1..DRONESIM_MAX_K + 1, c not in {2, 5}, M outside
 * 0..1024, m outside 1..4, weight not finite or < 0.                                                                               */
int dronesim_obstacle_observe(const float *z, const float *xF, const float *radius, const float *sense, const float *obstacles,
                              int R, int N, int k1, int c, int M, int m, float *x_out, float *cost_out, float weight, void *stream);
int dronesim_obstacle_reward(const float *z_post, const float *z_final, const uint8_t *done, const float *reward, const float *xF,
                             const float *radius, const float *sense, const float *obstacles, int T, int E, int N, int k1, int c, int M,
                             float weight, float *reward_out, float *cost_out, void *stream);
int dronesim_obstacle_sense(const float *z, const float *xF, const float *radius, const float *sense, const float *obstacles,
                            int E, int N, int k1, int c, int M, int m, float *orow, int32_t *oid, float *gap_min, uint8_t *hit,
                            void *stream);
int dronesim_action_shield_obstacles(const float *z, const int32_t *nbr, const float *act, const float *radius, float rate, float margin,
                                     float u_max, float dt, int E, int N, int k1, int c, float *act_out, uint8_t *intervened,
                                     float *correction, const float *orow, const int32_t *oid, int m, int M, float obstacle_rate,
                                     void *stream);
int dronesim_episode_obstacle_safety(const float *z, const float *z_final, const uint8_t *done, const float *xF, const float *radius,
                                     const float *obstacles, int T, int E, int N, int k1, int c, int M, int32_t *ep_len,
                                     float *min_obstacle_gap, int32_t *obstacle_hit_steps, float *ep_min_obstacle_gap,
                                     int32_t *ep_obstacle_hit_steps, void *stream);

const char *dronesim_last_error(void);
const char *dronesim_error_string(int code);
int dronesim_version(void);

#ifdef __cplusplus
}
#endif
#endif /* DRONESIM_H */
