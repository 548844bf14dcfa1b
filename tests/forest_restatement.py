"""The forest of `polee model random-forest` restated in NumPy and plain Python from its definition, not from the
C++: the bootstrap, the keyed bijection behind a node's candidate features, the builder and the votes.  Slow and literal on purpose."""
import math

import numpy as np

M32 = 0xFFFFFFFF
TAG_BOOT = 0x626F6F74
TAG_FEISTEL = 0x66656900


def philox4x32_10(c, seed):
    """one Philox4x32-10 block of the counter c (four 32-bit words) under the 64-bit key `seed`"""
    c0, c1, c2, c3 = c
    k0, k1 = seed & M32, (seed >> 32) & M32
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def bootstrap(seed, tree, N, Nb):
    """entry i = mulhi32(word 0 of the block (i, tag, 0, tree), N)"""
    return np.array([(philox4x32_10((i, TAG_BOOT, 0, tree), seed)[0] * N) >> 32 for i in range(Nb)], np.int64)


def candidate_feature(seed, tree, node, n, pos):
    """position `pos` of the bijection of [0, n) keyed by (seed, tree, node): a balanced 4-round Feistel network over b bits, b = the
    bit length of n - 1 rounded up to even (at least 2), cycle-walked until the value is below n"""
    b = max(2, (n - 1).bit_length())
    h = (b + 1) // 2
    mask = (1 << h) - 1
    v = pos
    while True:
        left, right = v >> h, v & mask
        for r in range(4):
            left, right = right, left ^ (philox4x32_10((right, TAG_FEISTEL + r, node, tree), seed)[0] & mask)
        v = (left << h) | right
        if v < n:
            return v


def nsub_of(n, nsubfeatures):
    return max(1, min(n, int(round(nsubfeatures * math.sqrt(n)))))  # (Python rounds half to even)


def nboot_of(N, partial_sampling):
    return max(1, int(math.floor(partial_sampling * N)))


def build_tree(x, labels, k, seed, tree, Nb, nsub, T, max_depth=-1, min_samples_leaf=1, min_samples_split=2):
    """one tree: lists feature, threshold, left, right, label, numbered level by level"""
    N, n = x.shape
    rows = bootstrap(seed, tree, N, Nb)
    feature, threshold, left, right, label = [-1], [0.0], [-1], [-1], [0]
    segs = [(rows, 0)]
    node = 0
    while node < len(segs):
        r, depth = segs[node]
        lab = labels[r]
        tot = np.bincount(lab, minlength=k)
        label[node] = int(np.argmax(tot))  # (the first maximum: the smallest class on a tie)
        cnt = len(r)
        if tot.max() == cnt or cnt < min_samples_split or depth == max_depth:
            node += 1
            continue
        best = None  # (score, threshold, feature)
        for pos in range(nsub):
            f = candidate_feature(seed, tree, node, n, pos)
            v = x[r, f]
            order = np.argsort(v, kind="stable")
            sv, sl = v[order], lab[order]
            if sv[0] == sv[-1]:
                continue
            cl = np.zeros(k, np.int64)
            for i in range(1, cnt):
                cl[sl[i - 1]] += 1
                if not (sv[i - 1] < sv[i]) or i < min_samples_leaf or cnt - i < min_samples_leaf:
                    continue
                s = 0.0
                for c in range(k):
                    s += T[cl[c]]
                    s += T[tot[c] - cl[c]]
                s -= T[i]
                s -= T[cnt - i]
                if best is None or s > best[0]:  # (positions and boundaries ascend: ties keep the first)
                    best = (s, (float(sv[i - 1]) + float(sv[i])) / 2, f)
        if best is not None:
            _, thr, f = best
            goes = x[r, f].astype(np.float64) < thr
            feature[node], threshold[node] = f, thr
            left[node], right[node] = len(segs), len(segs) + 1
            segs.append((r[goes], depth + 1))
            segs.append((r[~goes], depth + 1))
            for a in (feature, left, right):
                a.extend([-1, -1])
            threshold.extend([0.0, 0.0])
            label.extend([0, 0])
        node += 1
    return feature, threshold, left, right, label


def build_forest(x, labels, k, seed, ntrees=200, nsubfeatures=10.0, partial_sampling=1.0, max_depth=-1, min_samples_leaf=1,
                 min_samples_split=2):
    """(tree_off i64 [ntrees+1], feature i32, threshold f64, left i32, right i32, label i32)"""
    x = np.asarray(x, np.float32)
    labels = np.asarray(labels, np.int64)
    N, n = x.shape
    Nb, nsub = nboot_of(N, partial_sampling), nsub_of(n, nsubfeatures)
    T = [0.0] + [c * math.log(c) for c in range(1, Nb + 1)]
    off, cols = [0], [[], [], [], [], []]
    for t in range(ntrees):
        tree = build_tree(x, labels, k, seed, t, Nb, nsub, T, max_depth, min_samples_leaf, min_samples_split)
        for col, a in zip(cols, tree):
            col.extend(a)
        off.append(len(cols[0]))
    return (np.array(off, np.int64), np.array(cols[0], np.int32), np.array(cols[1], np.float64), np.array(cols[2], np.int32),
            np.array(cols[3], np.int32), np.array(cols[4], np.int32))


def votes(nodes, x, k):
    """i64 [R, k]: every tree votes the label of the leaf a row reaches; left iff (double)x < threshold"""
    off, feature, threshold, left, right, label = nodes
    x = np.asarray(x, np.float32)
    out = np.zeros((x.shape[0], k), np.int64)
    for r in range(x.shape[0]):
        for t in range(len(off) - 1):
            b, i = int(off[t]), 0
            while feature[b + i] >= 0:
                i = int(left[b + i]) if float(x[r, feature[b + i]]) < threshold[b + i] else int(right[b + i])
            out[r, label[b + i]] += 1
    return out


def planted_data(rng, N, n, k, signal=3, constant=4, shift=2.0):
    """rows N(0,1); class c adds `shift` on its own `signal` features; the last `constant` columns are constant"""
    labels = rng.integers(0, k, N)
    x = rng.normal(size=(N, n)).astype(np.float32)
    for c in range(k):
        cols = [(c * signal + j) % max(1, n - constant) for j in range(signal)]
        x[np.ix_(labels == c, cols)] += np.float32(shift)
    if constant and n > constant:
        x[:, n - constant:] = np.float32(0.25)
    return x, labels.astype(np.int32)
