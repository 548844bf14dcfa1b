"""NumPy / plain-Python restatement of the definition of `polee fit-tree` as this project fixes it:
the one-permutation MinHash sketch of a transcript's canonical 32-mers, the greedy Jaccard tree in its indexed form (a
heap plus a value -> nodes map, what the library's host builder does) and in its brute-force form (the best pair among all
active pairs, every step: the definition itself), the Huffman phase and the DFS serialisation.  The tests compare the
library against these; nothing here calls the library."""
import heapq

import numpy as np

K = 32
H = 200
_M64 = (1 << 64) - 1
_CODE = np.full(256, 4, np.uint8)
for _i, _c in enumerate("ACGT"):
    _CODE[ord(_c)] = _i
    _CODE[ord(_c.lower())] = _i


def mix64(c):
    """the hash of a packed canonical k-mer: uint64 array in, uint64 array out (arithmetic mod 2^64)"""
    with np.errstate(over="ignore"):
        z = c + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def sketch(seq):
    """seq: bytes / str -> uint64 [200]"""
    if isinstance(seq, str):
        seq = seq.encode("ascii", "replace")
    out = np.zeros(H, np.uint64)
    codes = _CODE[np.frombuffer(bytes(seq), np.uint8)]
    nw = len(codes) - K + 1
    if nw <= 0:
        return out
    bad = np.concatenate([[0], np.cumsum(codes > 3)])
    ok = (bad[K:] - bad[:-K]) == 0
    c2 = (codes & 3).astype(np.uint64)
    fw = np.zeros(nw, np.uint64)
    bw = np.zeros(nw, np.uint64)
    for j in range(K):
        fw |= c2[j:j + nw] << np.uint64(62 - 2 * j)
        bw |= (np.uint64(3) - c2[j:j + nw]) << np.uint64(2 * j)
    h = mix64(np.minimum(fw, bw)[ok])
    h = np.minimum(h, np.uint64(_M64 - 2))
    b = (h % np.uint64(H)).astype(np.int64)
    v = h + np.uint64(1)
    best = np.full(H, _M64, np.uint64)
    np.minimum.at(best, b, v)
    out[:] = np.where(best == np.uint64(_M64), np.uint64(0), best)
    return out


def sketches(seqs):
    return np.stack([sketch(s) for s in seqs]) if len(seqs) else np.zeros((0, H), np.uint64)


def similarity(a, b):
    """(mat, empt) of two sketches"""
    return int(((a == b) & (a != 0)).sum()), int(((a == 0) & (b == 0)).sum())


def jaccard(mat, empt):
    return float(np.float32(mat) / np.float32(H - empt))


def union(a, b):
    return np.where(a == 0, b, np.where(b == 0, a, np.minimum(a, b)))


def candidate_pairs(sk):
    """every pair (u < v, 1-based) of rows with mat > 0 -> sorted list of (u, v, mat, empt)"""
    where = {}
    for i, row in enumerate(sk):
        for val in row[row != 0].tolist():
            where.setdefault(val, []).append(i + 1)
    cnt = {}
    for nodes in where.values():
        for a in range(len(nodes)):
            for b in range(a + 1, len(nodes)):
                cnt[(nodes[a], nodes[b])] = cnt.get((nodes[a], nodes[b]), 0) + 1
    return [(u, v, m, similarity(sk[u - 1], sk[v - 1])[1]) for (u, v), m in sorted(cnt.items())]


def _finish(n, left, right, height, active):
    """Huffman phase over the active nodes, then order_nodes: (node_parent_idxs, node_js)"""
    heap = [(height[x], x) for x in active]
    heapq.heapify(heap)
    while len(heap) > 1:
        ha, a = heapq.heappop(heap)
        hb, b = heapq.heappop(heap)
        w = len(left)
        left.append(a); right.append(b); height.append(1 + max(ha, hb))
        heapq.heappush(heap, (height[w], w))
    root = heap[0][1]
    parents, js = [], []
    stack = [(root, 0)]
    while stack:
        node, par = stack.pop()
        idx = len(parents) + 1
        parents.append(par)
        if node <= n:
            js.append(node)
        else:
            js.append(0)
            stack.append((left[node], idx))   # left pushed first ...
            stack.append((right[node], idx))  # ... right popped first
    return np.array(parents, np.int32), np.array(js, np.int32)


def tree_indexed(sk, stats=None):
    """heap on (J desc, u, v) + value -> nodes map, extended after each merge"""
    n = len(sk)
    sks = [None] + [np.asarray(r, np.uint64) for r in sk]
    left, right, height = [0] * (n + 1), [0] * (n + 1), [0] * (n + 1)
    active = [False] + [True] * n
    where = {}
    for x in range(1, n + 1):
        for val in sks[x][sks[x] != 0].tolist():
            where.setdefault(val, []).append(x)
    first = candidate_pairs(sk)
    longest_run = max([len(v) for v in where.values()] + [0])
    heap = [(-jaccard(m, e), u, v) for u, v, m, e in first]
    heapq.heapify(heap)
    merges = 0
    while heap:
        _, u, v = heapq.heappop(heap)
        if not (active[u] and active[v]):
            continue
        w = len(sks)
        s = union(sks[u], sks[v])
        sks.append(s); left.append(u); right.append(v); height.append(1 + max(height[u], height[v]))
        active[u] = active[v] = False
        active.append(True)
        merges += 1
        cnt = {}
        for val in s[s != 0].tolist():
            for x in where[val]:
                if active[x]:
                    cnt[x] = cnt.get(x, 0) + 1
            where[val].append(w)
        for x, m in cnt.items():
            heapq.heappush(heap, (-jaccard(m, similarity(sks[x], s)[1]), x, w))
    rest = [x for x in range(1, len(sks)) if active[x]]
    if stats is not None:
        stats.update(initial_pairs=len(first), longest_run=longest_run, merges=merges, left_for_huffman=len(rest))
    p, j = _finish(n, left, right, height, rest)
    if stats is not None:
        stats.update(nodes=len(p), height=max(height))
    return p, j


def tree_brute(sk):
    """the definition: every step the best pair among all active pairs"""
    n = len(sk)
    sks = [None] + [np.asarray(r, np.uint64) for r in sk]
    left, right, height = [0] * (n + 1), [0] * (n + 1), [0] * (n + 1)
    act = list(range(1, n + 1))
    while True:
        best = None
        if len(act) > 1:
            A = np.stack([sks[x] for x in act])
            eq = (A[:, None, :] == A[None, :, :]) & (A[:, None, :] != 0)
            mat = eq.sum(axis=2)
            empt = ((A[:, None, :] == 0) & (A[None, :, :] == 0)).sum(axis=2)
            for a in range(len(act)):
                for b in range(a + 1, len(act)):
                    if mat[a, b] > 0:
                        key = (-jaccard(mat[a, b], empt[a, b]), act[a], act[b])
                        if best is None or key < best:
                            best = key
        if best is None:
            break
        _, u, v = best
        w = len(sks)
        sks.append(union(sks[u], sks[v])); left.append(u); right.append(v); height.append(1 + max(height[u], height[v]))
        act = [x for x in act if x != u and x != v] + [w]
    return _finish(n, left, right, height, act)


def revcomp(seq):
    comp = {"A": "T", "C": "G", "G": "C", "T": "A", "a": "t", "c": "g", "g": "c", "t": "a"}
    return "".join(comp.get(c, c) for c in reversed(seq))


def random_sketches(n, rng, pool=6, fill=0.7):
    """tie-heavy valid sketches: every bin draws from a small pool of values of that bin (or stays empty), then one row is
    duplicated and an all-zero row appended -> uint64 [n + 2][200]"""
    base = rng.integers(0, 1 << 40, size=(pool, H)).astype(np.uint64) * np.uint64(H) + np.arange(H, dtype=np.uint64)  # h' with h' % 200 == bin
    pick = rng.integers(0, pool, size=(n, H))
    sk = base[pick, np.arange(H)[None, :]] + np.uint64(1)
    sk[rng.random((n, H)) > fill] = 0
    if n > 2:  # a few sparse rows: few shared bins, many empty ones
        sk[rng.integers(0, n, size=max(1, n // 6))] *= (rng.random((max(1, n // 6), H)) < 0.05).astype(np.uint64)
    return np.concatenate([sk, sk[:1], np.zeros((1, H), np.uint64)])


TIE_CASES = [1, 2, 12, 25, 40, 60]


def tie_case(n):
    return random_sketches(n, np.random.default_rng(100 + n))


def valid_tree(parents, js, n):
    assert len(parents) == len(js) == 2 * n - 1 and parents[0] == 0
    assert sorted(js[js > 0].tolist()) == list(range(1, n + 1))  # every transcript is a leaf exactly once
    kids = np.bincount(parents[1:], minlength=2 * n)
    internal = np.flatnonzero(js == 0) + 1
    assert (kids[internal] == 2).all() and kids.sum() == 2 * n - 2
    assert (parents[1:] < np.arange(2, 2 * n)).all()  # parents precede children (DFS pre-order)
