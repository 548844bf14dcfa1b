"""NumPy / plain-Python restatement of the ROUNDS merge of `polee fit-tree` ("merge in rounds"): every
round merges each edge that is the best edge of both its endpoints under a total order of priorities.  Two forms: the
definition itself (all active pairs, every round) and the edge-list form the library computes (edges relabelled through
`into`, touched pairs de-duplicated and re-evaluated).  Sketches, similarity, union, the Huffman phase and the DFS are those of
kmer_tree_restatement; nothing here calls the library."""
import numpy as np

import kmer_tree_restatement as R

H = R.H
_M64 = (1 << 64) - 1


def h32(lo, hi):
    """the hash of an edge's endpoints (1-based node numbers, lo < hi): low 32 bits, arithmetic mod 2^64"""
    h = ((lo * 0x9E3779B97F4A7C15) & _M64) ^ ((hi * 0xC2B2AE3D27D4EB4F + 0x165667B19E3779F9) & _M64)
    h ^= h >> 29
    h = (h * 0xBF58476D1CE4E5B9) & _M64
    h ^= h >> 32
    return h & 0xFFFFFFFF


def jbits(mat, empt):
    """bit pattern of J = Float32(mat) / Float32(200 - empt)"""
    return int((np.float32(mat) / np.float32(H - empt)).view(np.uint32))


def priority(u, v, mat, empt):
    """larger = merged first: (J bits, hash, smaller u, smaller v)"""
    return (jbits(mat, empt), h32(u, v), -u, -v)


def _select(edges):
    """edges: {(u, v): priority} -> the edges that are the best of both endpoints, by descending priority"""
    best = {}
    for (u, v), p in edges.items():
        for x in (u, v):
            if x not in best or p > best[x][0]:
                best[x] = (p, (u, v))
    chosen = [(p, e) for e, p in edges.items() if best[e[0]][1] == e and best[e[1]][1] == e]
    chosen.sort(reverse=True)
    return [e for _, e in chosen]


def _apply(merges, sks, left, right, height, active):
    into = {}
    for u, v in merges:
        w = len(sks)
        sks.append(R.union(sks[u], sks[v])); left.append(u); right.append(v); height.append(1 + max(height[u], height[v]))
        active.discard(u); active.discard(v); active.add(w)
        into[u] = into[v] = w
    return into


def _start(sk):
    n = len(sk)
    sks = [None] + [np.asarray(r, np.uint64) for r in sk]
    return n, sks, [0] * (n + 1), [0] * (n + 1), [0] * (n + 1), set(range(1, n + 1))


def rounds_brute(sk, stats=None):
    """the definition: every round, the edges are all pairs of active nodes with mat > 0"""
    n, sks, left, right, height, active = _start(sk)
    per_round = []
    while len(active) > 1:
        act = sorted(active)
        A = np.stack([sks[x] for x in act])
        nz = A != 0
        mat = np.zeros((len(act), len(act)), np.int64)
        empt = np.zeros_like(mat)
        for a in range(len(act)):  # (row by row: the [a][a][200] cube of 320 nodes would be 20 MB of bools per round)
            mat[a] = ((A == A[a]) & nz[a]).sum(axis=1)
            empt[a] = (~nz & ~nz[a]).sum(axis=1)
        ia, ib = np.nonzero(np.triu(mat > 0, 1))
        edges = {(act[a], act[b]): priority(act[a], act[b], mat[a, b], empt[a, b]) for a, b in zip(ia.tolist(), ib.tolist())}
        if not edges:
            break
        merges = _select(edges)
        per_round.append(len(merges))
        _apply(merges, sks, left, right, height, active)
    if stats is not None:
        stats.update(rounds=len(per_round), merges=sum(per_round), left_for_huffman=len(active), per_round=per_round)
    out = R._finish(n, left, right, height, sorted(active))
    if stats is not None:
        stats.update(height=max(height))  # (of the whole tree: the Huffman phase extends the lists)
    return out


def rounds_indexed(sk, stats=None):
    """the edge-list form: after a round both endpoints of every edge go through `into`; an edge inside one new node vanishes, an
    untouched edge keeps its priority, the others are made canonical, de-duplicated and re-evaluated (dropped where mat = 0)"""
    n, sks, left, right, height, active = _start(sk)
    edges = {(u, v): priority(u, v, m, e) for u, v, m, e in R.candidate_pairs(sk)}
    per_round, reevaluated = [], 0
    while edges:
        merges = _select(edges)
        per_round.append(len(merges))
        into = _apply(merges, sks, left, right, height, active)
        kept, touched = {}, set()
        for (u, v), p in edges.items():
            a, b = into.get(u, u), into.get(v, v)
            if a == b:
                continue
            if a == u and b == v:
                kept[(u, v)] = p
            else:
                touched.add((min(a, b), max(a, b)))
        reevaluated += len(touched)
        for u, v in touched:
            m, e = R.similarity(sks[u], sks[v])
            if m > 0:
                kept[(u, v)] = priority(u, v, m, e)
        edges = kept
    if stats is not None:
        stats.update(rounds=len(per_round), merges=sum(per_round), left_for_huffman=len(active), reevaluated=reevaluated,
                     per_round=per_round)
    out = R._finish(n, left, right, height, sorted(active))
    if stats is not None:
        stats.update(height=max(height))  # (of the whole tree: the Huffman phase extends the lists)
    return out
