"""Model of the narrowed round check (zkfl_groth16_verify_round_narrow): which group a job falls
into, every group's expected value and the report's counts.

Grouping: the jobs are ordered by key (keys in order of first appearance, stable), the order is
cut into passes of `chunk` jobs (0 = 4096) and every pass into runs of `group` consecutive jobs
(0 = ROUND_GROUP, at most the pass size); the last group of a pass may be short, and groups are
numbered across passes.  A group's value is verify_round_model.expected_gt over its unscreened
jobs: the product of their check values raised to z_i.
"""
import verify_round_model as M

ROUND_GROUP = 64
PASS = 4096


def grouping(key_ids, chunk=0, group=0):
    """key_ids: one hashable per job -> (group_of per job, number of groups)."""
    n = len(key_ids)
    if n == 0:
        return [], 0
    first = {}
    for k in key_ids:
        first.setdefault(k, len(first))
    order = sorted(range(n), key=lambda i: first[key_ids[i]])  # stable
    size = min(n, chunk or PASS)
    group = group or min(ROUND_GROUP, size)
    assert 1 <= group <= size
    group_of, base = [None] * n, 0
    for off in range(0, n, size):
        m = min(size, n - off)
        for j in range(m):
            group_of[order[off + j]] = base + j // group
        base += (m + group - 1) // group
    return group_of, base


def expected_groups(jobs, zs, screened, chunk=0, group=0):
    """jobs: verify_round_model's [(vk, key_id, pub ints, proof bytes)]; screened: [bool] ->
    (group_of, [384 B per group])."""
    group_of, ng = grouping([j[1] for j in jobs], chunk, group)
    values = []
    for g in range(ng):
        mine = [i for i in range(len(jobs)) if group_of[i] == g and not screened[i]]
        values.append(M.expected_gt([jobs[i] for i in mine], [zs[i] for i in mine]))
    return group_of, values


def expected_report(key_ids, screened, valid, chunk=0, group=0):
    """valid: the per-job verdicts -> the report a narrowing call gives (without `keys`)."""
    group_of, ng = grouping(key_ids, chunk, group)
    n = len(key_ids)
    bad = {group_of[i] for i in range(n) if not screened[i] and not valid[i]}
    return {"screened": sum(map(bool, screened)), "combined": n - sum(map(bool, screened)),
            "passed": 0 if bad else 1, "groups": ng, "bad_groups": len(bad),
            "fallback": sum(1 for i in range(n) if not screened[i] and group_of[i] in bad)}
