"""The sketches the tests of the rounds merge run on (test_fit_tree_rounds_host.py, test_gpu_fit_tree_rounds.py), the crafted
edges of the selection step, and its plain-Python statement."""
import numpy as np

import kmer_tree_restatement as R

H = R.H


def _value(b, k):
    """a valid sketch value of bin b: h' = 200 k + b, stored as h' + 1"""
    return np.uint64(200 * k + b + 1)


def small_shapes():
    """name -> sketches: shapes at which the edge-list form can go wrong, each small enough to read"""
    rng = np.random.default_rng(77)
    cases = {}
    row = np.array([_value(b, 5 + b) if b % 3 else np.uint64(0) for b in range(H)], np.uint64)
    # two merges in round 1; the four old edges between the two new nodes must become ONE pair
    cases["four copies of one sketch"] = np.stack([row] * 4)
    # 65 pairs of duplicates, nothing shared between pairs: 65 merges in one round (more than a wave), numbered by the hash alone
    pairs = np.zeros((130, H), np.uint64)
    for i in range(65):
        r = np.array([_value(b, 1000 * (i + 1) + b) for b in range(H)], np.uint64)
        r[rng.random(H) > 0.6] = 0
        pairs[2 * i] = pairs[2 * i + 1] = r
    cases["65 disjoint duplicate pairs"] = pairs[rng.permutation(130)]
    # values only in the last eight bins: the tail of the 64-wide strides
    tail = np.zeros((9, H), np.uint64)
    for t in range(9):
        for b in range(192, 200):
            if rng.random() < 0.8:
                tail[t, b] = _value(b, int(rng.integers(1, 3)))
    tail[0, 192:200] = [_value(b, 1) for b in range(192, 200)]
    cases["values only in bins 192-199"] = tail
    full = np.array([_value(b, 7) for b in range(H)], np.uint64)
    single = np.zeros(H, np.uint64)
    single[131] = _value(131, 7)
    cases["all 200 bins against a single bin"] = np.stack([full, single])
    cases["n = 2, nothing shared"] = np.stack([full, np.array([_value(b, 8) for b in range(H)], np.uint64)])
    return cases


def all_cases(P, fixture_seqs):
    """name -> sketches: the tie-heavy sets, the edge cases of test_gpu_fit_tree (fixture, one value shared by 300, duplicates and
    empty rows, all empty, n = 1) and the small shapes"""
    from test_gpu_fit_tree import _edge_cases
    cases = dict(_edge_cases(P, fixture_seqs))
    for n in R.TIE_CASES:
        cases["ties %d" % n] = R.tie_case(n)
    cases.update(small_shapes())
    return cases


K = 0x3F00000012345678  # a key as the builders form it: bits of J = 0.5, some hash


def crafted_selections():
    """name -> (num_nodes, u, v, key, merged edges in the order of their priorities)"""
    out = {}
    # equal 64-bit keys at node 1: the smaller (lo, hi) wins, so (1, 2) and not (1, 3); (1, 3) is the best of 3, (3, 4) the best of 4:
    # neither is merged.  (5, 6) has a larger key: first.  (7, 8) has the key of (1, 2): after it, by the smaller pair.
    out["equal keys at one node"] = (8, [3, 1, 7, 1, 5], [4, 3, 8, 2, 6], [K - 1, K, K, K, K + 5], [(5, 6), (1, 2), (7, 8)])
    # a path 1 - 2 - 3 - 4 with keys 5, 9, 7: the middle edge is the best of both its endpoints; the outer ones of one each
    out["three-edge path"] = (4, [1, 2, 3], [2, 3, 4], [5, 9, 7], [(2, 3)])
    # a star whose edges all have one key: the centre takes the smallest pair, the other leaves stay
    out["star of equal keys"] = (6, [2, 2, 1, 2, 2], [6, 4, 2, 3, 5], [K] * 5, [(1, 2)])
    return out


def random_selection(rng, num_nodes=3000, E=20000, keys=40):
    """many edges, few distinct keys: several blocks, ties at most nodes"""
    pairs = set()
    while len(pairs) < E:
        a, b = rng.integers(1, num_nodes + 1, 2)
        if a != b:
            pairs.add((int(min(a, b)), int(max(a, b))))
    pairs = sorted(pairs)
    order = rng.permutation(E)
    u = np.array([pairs[i][0] for i in order], np.uint32)
    v = np.array([pairs[i][1] for i in order], np.uint32)
    key = (np.uint64(K) + rng.integers(0, keys, E).astype(np.uint64))
    return num_nodes, u, v, key


def select_reference(u, v, key):
    """the definition of the selection step: (merged uint8 [E], order int32 [E])"""
    pri = [(int(k), -int(a), -int(b)) for a, b, k in zip(u, v, key)]
    best = {}
    for e, (a, b) in enumerate(zip(u.tolist(), v.tolist())):
        for x in (a, b):
            if x not in best or pri[e] > pri[best[x]]:
                best[x] = e
    chosen = sorted((e for e, (a, b) in enumerate(zip(u.tolist(), v.tolist())) if best[a] == e and best[b] == e), key=lambda e: pri[e], reverse=True)
    merged, order = np.zeros(len(u), np.uint8), np.full(len(u), -1, np.int32)
    for q, e in enumerate(chosen):
        merged[e], order[e] = 1, q
    return merged, order
