// Host-side pieces shared by the entry points that read observation records z [..][N][k1][c] (shield.hip, obstacles.hip, env_obstacles.hip,
// evaluate.hip): the load-width rule of their kernels and the checks of the arguments they have in common.  Every check returns
// DRONESIM_OK or fails under the entry's own name (`where`), so an entry states only the order of its checks and its own ones.
#pragma once
#include <limits.h>
#include "common.hpp"
#include "dronesim_env_obstacles.h"

// Floats per load of a record's rows: 4 (c = 2, k1 even, 16-byte aligned: two rows per load), 2 (c = 2, 8-byte aligned: one row per
// load) or 1.  `addresses`: the OR of the bases of every array of records the kernel reads (z, and z_final where there is one).
inline int record_load_width(int k1, int c, uintptr_t addresses)
{
    if (c != 2) return 1;
    if ((k1 % 2) == 0 && (addresses & 15u) == 0) return 4;
    return (addresses & 7u) == 0 ? 2 : 1;
}

// the record geometry; k1_min / k1_max: the entry's own bounds (INT_MAX: none)
inline int check_records(const char *where, int N, int k1, int k1_min, int k1_max, int c)
{
    if (N >= 1 && N <= DRONESIM_MAX_AGENTS && k1 >= k1_min && k1 <= k1_max && (c == 2 || c == 5)) return DRONESIM_OK;
    char what[96];
    if (k1_max == INT_MAX) snprintf(what, sizeof what, "N outside 1..%d, k1 < %d or c not in {2, 5}", DRONESIM_MAX_AGENTS, k1_min);
    else snprintf(what, sizeof what, "N outside 1..%d, k1 outside %d..%d or c not in {2, 5}", DRONESIM_MAX_AGENTS, k1_min, k1_max);
    return fail_at(where, what);
}

// the disc count, and the list [M][3] where the entry reads it: `obstacles` = its argument, or nullptr with reads_list = false for an
// entry that has no such argument (the shield reads the sensed rows)
inline int check_discs(const char *where, int M, const float *obstacles, bool reads_list = true)
{
    if (M >= 0 && M <= DRONESIM_MAX_OBSTACLES && (M == 0 || obstacles || !reads_list)) return DRONESIM_OK;
    char what[96];
    if (reads_list) snprintf(what, sizeof what, "M outside 0..%d, or NULL obstacles with M > 0", DRONESIM_MAX_OBSTACLES);
    else snprintf(what, sizeof what, "M outside 0..%d", DRONESIM_MAX_OBSTACLES);
    return fail_at(where, what);
}

// the per-env lists [E][M][3] (include/dronesim_env_obstacles.h): the row count M of every env, and the lists where M > 0; the
// counts [E] may be NULL (every env holds M discs), their VALUES are device data and are clamped by the kernels
inline int check_env_discs(const char *where, int M, const float *obstacles)
{
    if (M >= 0 && M <= DRONESIM_MAX_ENV_OBSTACLES && (M == 0 || obstacles)) return DRONESIM_OK;
    char what[96];
    snprintf(what, sizeof what, "M outside 0..%d, or NULL obstacles with M > 0", DRONESIM_MAX_ENV_OBSTACLES);
    return fail_at(where, what);
}

// slots of the per-agent obstacle list
inline int check_slots(const char *where, int m)
{
    if (m >= 1 && m <= DRONESIM_MAX_SENSE) return DRONESIM_OK;
    char what[48];
    snprintf(what, sizeof what, "m outside 1..%d", DRONESIM_MAX_SENSE);
    return fail_at(where, what);
}

// the obstacle cost's weight: finite, not NaN, >= 0
inline int check_weight(const char *where, float weight)
{
    return weight >= 0.0f && weight <= 3.402823466e38f ? DRONESIM_OK : fail_at(where, "weight must be finite and >= 0");
}
