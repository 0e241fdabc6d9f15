"""CPU: the chunk planner of the four batch registration tools (host/RegistrationChunks.h through tests/hostcheck) against a
restatement of its rule in Python: starting with no files, a match adds its query if new, then every file of its clipped window
that is new and is not the query, ascending; it joins the chunk only if the files stay within the limit.  Chunk boundaries, file
order, match table, map_offs and entry_frame are compared for equality over whole match lists."""
import numpy as np
import pytest

import hostcheck_lib as hc


def _window(m, half, lo, hi):
    return range(max(lo, m - half), min(hi, m + half) + 1)


def _plan(matches, m0, half, lo, hi, limit, maps):
    local = {}
    m1 = m0
    while m1 < len(matches):
        q, m, _ = matches[m1]
        add = ([] if q in local else [q]) + [j for j in _window(m, half, lo, hi) if j not in local and j != q]
        if len(local) + len(add) > limit:
            break
        for f in add:
            local[f] = len(local)
        m1 += 1
    chunk = matches[m0:m1]
    if not maps:
        return m1, list(local), [(local[q], local[m], a) for q, m, a in chunk], None, None
    entries = [[local[j] for j in _window(m, half, lo, hi)] for _, m, _ in chunk]
    offs = np.cumsum([0] + [len(e) for e in entries]).tolist()
    return m1, list(local), [(local[q], k, a) for k, (q, _, a) in enumerate(chunk)], offs, [f for e in entries for f in e]


def _frame_tools_rule(matches, m0, limit):
    """the frame tools' own wording: a match counts its query and its target, the target once if it is the query"""
    local = {}
    m1 = m0
    while m1 < len(matches):
        q, m, _ = matches[m1]
        add = (0 if q in local else 1) + (0 if m in local or m == q else 1)
        if len(local) + add > limit:
            break
        for f in (q, m):
            local.setdefault(f, len(local))
        m1 += 1
    return m1, list(local), [(local[q], local[m], a) for q, m, a in matches[m0:m1]], None, None


def _chunks(plan, matches, *args):
    out, m0 = [], 0
    while m0 < len(matches):
        c = plan(matches, m0, *args)
        assert c[0] > m0, "an admitted limit holds every single match"
        out.append(c)
        m0 = c[0]
    return out


def _random_matches(rng, n_files, n):
    rows = []
    for _ in range(n):
        kind = rng.integers(0, 6)
        if kind == 0 and rows:
            rows.append(rows[rng.integers(0, len(rows))])                      # a repeated match
            continue
        q = int(rng.integers(0, n_files))
        m = q if kind == 1 else int(rng.choice([0, n_files - 1])) if kind == 2 else int(rng.integers(0, n_files))
        rows.append((q, m, float(np.float32(rng.uniform(-180, 180)))))
    return rows


@pytest.mark.parametrize("half", [0, 1, 3])
def test_planner_equals_the_rule_on_random_lists(half):
    rng = np.random.default_rng(1000 + half)
    seen = dict(self=0, repeat=0, clip_lo=0, clip_hi=0, many=0)
    for _ in range(60):
        n_files = int(rng.integers(1, 13))
        matches = _random_matches(rng, n_files, int(rng.integers(1, 41)))
        for limit in range(2 * half + 2, 13):
            got = _chunks(hc.plan_chunk, matches, half, 0, n_files - 1, limit, True)
            assert got == _chunks(_plan, matches, half, 0, n_files - 1, limit, True), (matches, n_files, limit)
            seen["many"] += len(got) > 1
        seen["self"] += any(q == m for q, m, _ in matches)
        seen["repeat"] += len(set(matches)) < len(matches)
        seen["clip_lo"] += any(m - half < 0 for _, m, _ in matches)
        seen["clip_hi"] += any(m + half > n_files - 1 for _, m, _ in matches)
    assert all(v > 0 for k, v in seen.items() if half or not k.startswith("clip")), seen


def test_half_0_without_clipping_is_the_frame_tools_rule():
    rng = np.random.default_rng(77)
    lo, hi = hc.NO_CLIP
    for _ in range(40):
        names = rng.choice(100000, 12, replace=False)                          # file numbers, not places in a listing
        matches = [(int(names[q]), int(names[m]), a) for q, m, a in _random_matches(rng, 12, int(rng.integers(1, 41)))]
        for limit in range(2, 13):
            got = _chunks(hc.plan_chunk, matches, 0, lo, hi, limit, False)
            assert got == _chunks(_frame_tools_rule, matches, limit)
            assert got == _chunks(_plan, matches, 0, lo, hi, limit, False)
    fixed = [(7, 9, 1.0), (9, 7, 2.0), (5, 5, 3.0), (7, 5, 4.0), (11, 3, 5.0), (3, 11, 6.0)]
    got = _chunks(hc.plan_chunk, fixed, 0, lo, hi, 3, False)
    assert got == [(4, [7, 9, 5], [(0, 1, 1.0), (1, 0, 2.0), (2, 2, 3.0), (0, 2, 4.0)], None, None),
                   (6, [11, 3], [(0, 1, 5.0), (1, 0, 6.0)], None, None)]


def test_a_limit_that_holds_one_match_per_chunk():
    """12 files, half 1, the least limit 4: consecutive matches share too little to fit together"""
    matches = [(0, 4, 1.0), (8, 11, 2.0), (2, 0, 3.0), (6, 6, 4.0), (11, 8, 5.0)]
    got = _chunks(hc.plan_chunk, matches, 1, 0, 11, 4, True)
    assert got == [(1, [0, 3, 4, 5], [(0, 0, 1.0)], [0, 3], [1, 2, 3]),
                   (2, [8, 10, 11], [(0, 0, 2.0)], [0, 2], [1, 2]),                 # clipped above
                   (3, [2, 0, 1], [(0, 0, 3.0)], [0, 2], [1, 2]),                   # clipped below
                   (4, [6, 5, 7], [(0, 0, 4.0)], [0, 3], [1, 0, 2]),                # the query inside its own window
                   (5, [11, 7, 8, 9], [(0, 0, 5.0)], [0, 3], [1, 2, 3])]
    assert got == _chunks(_plan, matches, 1, 0, 11, 4, True)
