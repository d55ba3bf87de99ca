/*
 * dronesim_env_obstacles.h -- per-env obstacle sets: the obstacle entries of dronesim.h with a disc list PER ENV in place of the
 * one list all envs share.  A product header: libdronesim.so exports these symbols (csrc/env_obstacles.hip).  Conventions,
 * error codes, dronesim_last_error() and the stream argument are dronesim.h's.
 *
 * Inputs: obstacles [E][M][3] float32 (x, y, r), env e's list at obstacles + 3 M e; count [E] int32 or NULL (NULL: every env holds
 * M discs).  0 <= M <= DRONESIM_MAX_ENV_OBSTACLES (obstacles may be NULL at M = 0), 0 <= count[e] <= M: env e's discs are rows
 * 0..count[e]-1 of its list and ids are env-local.  Every kernel clamps count[e] into 0..M before it loops, so a bad count never
 * reads past the env's rows, and a row at or beyond count[e] is never read for its value.
 * xF [N][2] the goals; radius [N]; sense [N] the range of every agent -- shared by all envs, as in dronesim.h.
 *
 * The rule is dronesim.h's, with env e's own list in place of the shared one:
 * Position, from the agent's OWN record (row 0 is x_i - xF_i; c = 2 or 5): x = fl32(z[0] + xF[i][0]), y = fl32(z[1] + xF[i][1]).
 * Gap to disc o of env e: p = o.xy - (x, y), d = sqrtf(fmaf(p.y, p.y, p.x p.x)) (the correctly rounded square root),
 * gap = (d - radius[i]) - o.r -- the ONE float32 expression of the shared entries (csrc/obstacle_common.hpp), so every output
 * below is bit-identical to the shared entry run on env e's records with env e's first count[e] discs as its list.
 * List: among the discs with gap <= sense[i] (a NaN gap is not in range) the m smallest, 1 <= m <= DRONESIM_MAX_SENSE, by gap
 * ascending, then id ascending; slot s = (p.x, p.y, o.r) and the id, empty slots (0, 0, 0) and -1.
 * Cost: over ALL count[e] discs in ascending id, in float32: 9.99e3 where gap <= 0; logf(sense[i] / gap) where
 * 0 < gap <= sense[i]; 0 otherwise; cost = fl32(weight sum); no discs give 0.
 *
 * dronesim_env_obstacle_sense, per record (e, i) of z [E][N][k1 c]: orow [E][N][m][3], oid [E][N][m], and the optional planes
 * over ALL of env e's discs gap_min [E][N] (a NaN stays; +inf without discs) and hit [E][N] uint8 = gap_min <= 0.
 * dronesim_env_obstacle_observe takes R rows of [N][k1 c] with R % E == 0; row q belongs to env q % E (one step [E], a window ring
 * [T+1][E], the truncated ends [M_t][E] pass without a copy).  It writes x_out [R][N][k1 c + 3 m] -- the record's own bits, then
 * the list slots -- and, where cost_out is not NULL, cost_out [R][N].
 * dronesim_env_obstacle_reward is elementwise over (t, e, i) of z_post / z_final [T][E][N][k1 c], done [T][E], reward [T][E][N]:
 * reward_out = fl32(reward - cost(observation after step t)), the observation being z_final[t] where done[t] and z_final is
 * given, z_post[t] otherwise; reward_out == reward is allowed; cost_out [T][E][N] and z_final may be NULL.
 * dronesim_episode_env_obstacle_safety: the five tables of dronesim_episode_obstacle_safety (the FIRST episode of every env of
 * z [T][E][N][k1 c], done [T][E]; ep_len, min_obstacle_gap, obstacle_hit_steps, ep_min_obstacle_gap, ep_obstacle_hit_steps;
 * L_e = 0: NaN / 0; an env without discs: +inf / 0), one list per env for the whole window.
 *
 * One launch each (the tables: two with per-env tables), one thread per record or column, a 256-record workgroup.  A workgroup
 * touches up to 254 / N + 2 rows (envs) -- wrapping from env E-1 to env 0 where the leading dims are rows -- and its lanes reach
 * their lists by one of two paths, chosen on the host by dronesim_env_obstacle_plan from (N, M) alone:
 *   staged  the workgroup copies the lists of its rows into dynamic LDS, slot j = env (row_lo + j) % E at an odd slot stride (so
 *           that the envs of a wave fall into different banks), and a lane reads slot row - row_lo: lanes of one env broadcast;
 *   direct  every lane loads its env's disc from global memory: one address per env a wave spans, no LDS for the list.
 * Both give the same bits.  No atomics, no workspace, no host synchronisation: graph-capturable, bit-identical run to run.
 * E = 0 / R = 0 / T E = 0 enqueues nothing.
 *
 * dronesim_env_obstacle_plan (host only, no stream, usable without a GPU): *staged = 1 / 0, *rows_per_block = 254 / N + 2,
 * *lds_bytes = the most LDS a workgroup of these kernels holds for (N, M, m): the staged lists (0 on the direct path) plus the
 * 256 x 12 m bytes dronesim_env_obstacle_observe parks its output lists in.  Any of the three pointers may be NULL.
 *
 * EINVAL: what the shared entry refuses, with M outside 0..DRONESIM_MAX_ENV_OBSTACLES (or NULL obstacles with M > 0) in place of
 * its bound, and E < 1 with R > 0 or R % E != 0 for the observe entry.
 */
#ifndef DRONESIM_ENV_OBSTACLES_H
#define DRONESIM_ENV_OBSTACLES_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DRONESIM_MAX_ENV_OBSTACLES 64  /* discs of ONE env's list */

int dronesim_env_obstacle_plan(int N, int M, int m, int *staged, int *rows_per_block, size_t *lds_bytes);
int dronesim_env_obstacle_sense(const float *z, const float *xF, const float *radius, const float *sense, const float *obstacles,
                                const int32_t *count, int E, int N, int k1, int c, int M, int m, float *orow, int32_t *oid,
                                float *gap_min, uint8_t *hit, void *stream);
int dronesim_env_obstacle_observe(const float *z, const float *xF, const float *radius, const float *sense, const float *obstacles,
                                  const int32_t *count, int R, int E, int N, int k1, int c, int M, int m, float *x_out,
                                  float *cost_out, float weight, void *stream);
int dronesim_env_obstacle_reward(const float *z_post, const float *z_final, const uint8_t *done, const float *reward, const float *xF,
                                 const float *radius, const float *sense, const float *obstacles, const int32_t *count, int T, int E,
                                 int N, int k1, int c, int M, float weight, float *reward_out, float *cost_out, void *stream);
int dronesim_episode_env_obstacle_safety(const float *z, const float *z_final, const uint8_t *done, const float *xF,
                                         const float *radius, const float *obstacles, const int32_t *count, int T, int E, int N,
                                         int k1, int c, int M, int32_t *ep_len, float *min_obstacle_gap, int32_t *obstacle_hit_steps,
                                         float *ep_min_obstacle_gap, int32_t *ep_obstacle_hit_steps, void *stream);

#ifdef __cplusplus
}
#endif
#endif
