"""The argument-validation cases of the entries that read observation records (shield, obstacles, the safety tables), shared by
tests/test_record_entries_host.py and tests/golden/gen_record_entries.py.  No case reaches a launch: the baseline of every entry is a
valid EMPTY batch with fake non-null pointers, and a case with a non-empty batch is one that validation must refuse.

Per entry: `base` (every argument by name, in the header's order), `checks` (the entry's checks in the order the library makes them,
each with its single violations; the first one stands for the check in the pair cases) and `ok` (variations that stay valid)."""
import collections

P = 4096                                        # a fake device address: never dereferenced, nothing here launches
NAN, INF = float("nan"), float("inf")
Entry = collections.namedtuple("Entry", "base checks ok")
Case = collections.namedtuple("Case", "entry label args pair")        # pair: the labels of the two single cases it combines, or None


def _nulls(*names):
    return [(f"{n}=NULL", {n: 0}) for n in names]


def _values(name, *values):
    return [(f"{name}={v}", {name: v}) for v in values]


_RECORDS = _values("N", 0, 1025) + _values("c", 1, 3, 4, 6)
_RECORDS_OK = _values("N", 1, 1024) + _values("c", 5)
_DISCS = _values("M", -1, 1025)
_SLOTS = _values("m", 0, 5)
_WEIGHT = _values("weight", -1.0, NAN, INF, -INF)
_SHIELD_BASE = dict(z=P, nbr=P, act=P, radius=P, rate=0.5, margin=0.0, u_max=1.0, dt=0.05, E=0, N=4, k1=3, c=2, act_out=P,
                    intervened=P, correction=P)
_SHIELD_HEAD = [("batch", _values("E", -1)), ("records", _RECORDS + _values("k1", 1, 10))]
_SHIELD_RATE = ("rate", _values("rate", 0.0, -0.1, 0.5000001, NAN, INF, -INF))
_SHIELD_TAIL = [("margin", _values("margin", -1e-3, NAN, INF, -INF)), ("u_max", _values("u_max", 0.0, -1.0, NAN, -INF)),
                ("dt", _values("dt", 0.0, -0.05, NAN, INF))]
_SHIELD_OK = _RECORDS_OK + _values("k1", 2, 9) + _values("u_max", INF) + _values("rate", 1e-6) + _nulls("intervened", "correction")
_SENSE_BASE = dict(z=P, xF=P, radius=P, sense=P, obstacles=P)
_SENSE_DISCS = _DISCS + [("obstacles=NULL", {"obstacles": 0})]
_SENSE_OK = _RECORDS_OK + _values("k1", 1, 9) + _values("M", 1024) + [("M=0,obstacles=NULL", {"M": 0, "obstacles": 0})] + _values("m", 1, 4)

ENTRIES = {
    "dronesim_action_shield": Entry(
        _SHIELD_BASE,
        [("null", _nulls("z", "nbr", "act", "radius", "act_out"))] + _SHIELD_HEAD + [_SHIELD_RATE] + _SHIELD_TAIL,
        _SHIELD_OK),
    "dronesim_action_shield_obstacles": Entry(
        dict(_SHIELD_BASE, orow=P, oid=P, m=2, M=3, obstacle_rate=1.0),
        [("null", _nulls("z", "nbr", "act", "radius", "act_out", "orow", "oid"))] + _SHIELD_HEAD + [("slots", _SLOTS), ("discs", _DISCS),
         _SHIELD_RATE, ("obstacle_rate", _values("obstacle_rate", 0.0, -1.0, 1.0000001, NAN, INF, -INF))] + _SHIELD_TAIL,
        _SHIELD_OK + _values("m", 1, 4) + _values("M", 0, 1024) + _values("obstacle_rate", 1e-6)),
    "dronesim_shield_totals": Entry(
        dict(intervened=P, correction=P, E=0, N=4, interventions=P, nonfinite=P, correction_sum=P, correction_max=P),
        [("null", _nulls("intervened", "correction", "interventions", "nonfinite", "correction_sum", "correction_max")),
         ("batch", _values("E", -1)), ("agents", _values("N", 0, 1025))],
        _values("N", 1, 1024)),
    "dronesim_obstacle_sense": Entry(
        dict(_SENSE_BASE, E=0, N=4, k1=3, c=2, M=3, m=2, orow=P, oid=P, gap_min=P, hit=P),
        [("null", _nulls("z", "xF", "radius", "sense", "orow", "oid")), ("batch", _values("E", -1)),
         ("records", _RECORDS + _values("k1", 0, 10)), ("discs", _SENSE_DISCS), ("slots", _SLOTS)],
        _SENSE_OK + _nulls("gap_min", "hit")),
    "dronesim_obstacle_observe": Entry(
        dict(_SENSE_BASE, R=0, N=4, k1=3, c=2, M=3, m=2, x_out=P, cost_out=P, weight=1.0),
        [("null", _nulls("z", "xF", "radius", "sense", "x_out")), ("batch", _values("R", -1)),
         ("records", _RECORDS + _values("k1", 0, 10)), ("discs", _SENSE_DISCS), ("slots", _SLOTS), ("weight", _WEIGHT)],
        _SENSE_OK + _nulls("cost_out") + _values("weight", 0.0)),
    "dronesim_obstacle_reward": Entry(
        dict(z_post=P, z_final=P, done=P, reward=P, xF=P, radius=P, sense=P, obstacles=P, T=0, E=0, N=4, k1=3, c=2, M=3, weight=1.0,
             reward_out=P, cost_out=P),
        [("null", _nulls("z_post", "done", "reward", "xF", "radius", "sense", "reward_out")), ("batch", _values("T", -1) + _values("E", -1)),
         ("records", _RECORDS + _values("k1", 0, 10)), ("discs", _SENSE_DISCS), ("weight", _WEIGHT)],
        _RECORDS_OK + _values("k1", 1, 9) + _values("M", 1024) + [("M=0,obstacles=NULL", {"M": 0, "obstacles": 0})] + _nulls("z_final", "cost_out")
        + _values("weight", 0.0) + _values("T", 3) + _values("E", 3)),
    # (the window's pointers are checked behind the empty batch's return: their cases carry E = 1, and T = 1 where z / done are read)
    "dronesim_episode_obstacle_safety": Entry(
        dict(z=P, z_final=P, done=P, xF=P, radius=P, obstacles=P, T=2, E=0, N=4, k1=3, c=2, M=3, ep_len=P, min_obstacle_gap=P,
             obstacle_hit_steps=P, ep_min_obstacle_gap=P, ep_obstacle_hit_steps=P),
        [("batch", _values("T", -1) + _values("E", -1)), ("records", _RECORDS + _values("k1", 0)), ("discs", _SENSE_DISCS),
         ("tables", _nulls("min_obstacle_gap", "obstacle_hit_steps")),
         ("null", [(f"{n}=NULL,E=1", {n: 0, "E": 1}) for n in ("xF", "radius", "ep_len", "z", "done")])],
        _RECORDS_OK + _values("k1", 1, 100) + _values("M", 1024) + [("M=0,obstacles=NULL", {"M": 0, "obstacles": 0})] + _nulls("z_final")
        + [("every pointer NULL", dict(z=0, z_final=0, done=0, xF=0, radius=0, ep_len=0, min_obstacle_gap=0, obstacle_hit_steps=0,
                                       ep_min_obstacle_gap=0, ep_obstacle_hit_steps=0)),
           ("no per-env tables", dict(ep_min_obstacle_gap=0, ep_obstacle_hit_steps=0, min_obstacle_gap=0, obstacle_hit_steps=0))]),
    "dronesim_episode_safety": Entry(
        dict(z=P, nbr=P, z_final=P, nbr_final=P, done=P, radius=P, delta=P, done_radius=0.2, T=2, E=0, N=4, k1=3, c=2, ep_len=P,
             min_clearance=P, goal_dist_final=P, arrive_step=P, ep_min_clearance=P, ep_goal_dist_max=P, ep_arrived=P),
        [("null", _nulls("z", "nbr", "done", "radius", "delta", "ep_len")), ("batch", _values("T", -1) + _values("E", -1)),
         ("records", _RECORDS + _values("k1", 1)), ("done_radius", _values("done_radius", NAN)),
         ("finals", _nulls("z_final", "nbr_final")),
         ("tables", _nulls("min_clearance", "goal_dist_final")
          + [("goal_dist_final=NULL,ep_goal_dist_max=NULL", {"goal_dist_final": 0, "ep_goal_dist_max": 0}),
             ("goal_dist_final=NULL,ep_arrived=NULL", {"goal_dist_final": 0, "ep_arrived": 0})])],
        _RECORDS_OK + _values("k1", 2, 100) + _values("done_radius", INF, -1.0) + _values("T", 0) + _nulls("arrive_step")
        + [("no finals", dict(z_final=0, nbr_final=0)),
           ("no tables", dict(min_clearance=0, goal_dist_final=0, arrive_step=0, ep_min_clearance=0, ep_goal_dist_max=0, ep_arrived=0))]),
}


# Pairs beyond the adjacent first violations, as (check, label) of two single cases of the entry: the obstacle shield states its NULL
# check in two steps (the shared pointers, then orow / oid), and the second step must still stand in front of the batch check.
EXTRA_PAIRS = {"dronesim_action_shield_obstacles": [(("null", "orow=NULL"), ("batch", "E=-1")), (("null", "oid=NULL"), ("records", "N=0"))]}


def cases():
    """Every case, in a fixed order: the baseline, the valid variations, every single violation, one pair per adjacent pair of checks."""
    out = []
    for name, e in ENTRIES.items():
        out.append(Case(name, "baseline", dict(e.base), None))
        for kind, group in [("ok", e.ok)] + e.checks:
            for label, over in group:
                assert set(over) <= set(e.base), (name, label)
                out.append(Case(name, f"{kind}: {label}", dict(e.base, **over), None))
        for (ka, ga), (kb, gb) in zip(e.checks, e.checks[1:]):
            (la, oa), (lb, ob) = ga[0], gb[0]
            assert not set(oa) & set(ob), (name, la, lb)
            out.append(Case(name, f"pair: {la} + {lb}", dict(e.base, **oa, **ob), (f"{ka}: {la}", f"{kb}: {lb}")))
        for (ka, la), (kb, lb) in EXTRA_PAIRS.get(name, ()):
            oa, ob = dict(dict(e.checks)[ka])[la], dict(dict(e.checks)[kb])[lb]
            out.append(Case(name, f"pair: {la} + {lb}", dict(e.base, **oa, **ob), (f"{ka}: {la}", f"{kb}: {lb}")))
    return out


def run(lib, case):
    """(return code, message) of one case; the message is read only behind a failure (the string of an earlier one stays otherwise)."""
    rc = getattr(lib, case.entry)(*case.args.values(), None)
    return rc, (lib.dronesim_last_error().decode() if rc != 0 else "")
