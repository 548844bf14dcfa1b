"""NumPy restatement of the bias model trainer (src/bias.jl of the reference, line by line) with this project's three deviations
(DESIGN.md section 3.16): positions beyond a transcript's ends and the drawn background positions are Philox4x32-10 draws, and the
loss takes log in f64 and sums it in a fixed order (chunks of 256 by a halving tree, then the chunks in sequence).  Shared by
tests/test_bias_train_host.py and tests/test_gpu_bias_train.py; not a test module itself."""
import functools
import math

import numpy as np

K, MAXORDER, CTX = 20, 6, 4096
TAG_PAD, TAG_BG = 0x62706164, 0x62626764
f32 = np.float32


# ---- Philox4x32-10 (rng.hpp: philox4x32_10) ----------------------------------------------------------------------------------
def philox(c0, c1, c2, c3, seed):
    c = [np.asarray(x, np.uint64) & np.uint64(0xFFFFFFFF) for x in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    M = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        c = [((p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0)) & M, p1 & M, ((p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1)) & M, p0 & M]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c


def pad_nt(seed, i, cls, off):
    return int(philox(i, cls, off, TAG_PAD, seed)[0]) & 3


def bg_tpos(seed, i, span):
    r = philox(np.asarray(i), 0, 0, TAG_BG, seed)[0]
    return 1 + ((r * np.asarray(span, np.uint64)) >> np.uint64(32)).astype(np.int64)


# ---- BiasTrainingExample (bias.jl:21-101) ---------------------------------------------------------------------------------------
def make_example(ts, tpos, fl, seed, i, cls):
    """ts: the transcript's codes; -> (left [20], right [20], frag_gc)"""
    first, last = tpos - 5, tpos + fl - 1 + 5  # extract_padded_seq(tseq, first, last), 1-based inclusive
    frag = []
    for off, p in enumerate(range(first, last + 1)):
        if p < 1 or p > len(ts):
            frag.append(pad_nt(seed, i, cls, off))  # randdna()
        else:
            frag.append(int(ts[p - 1]) if ts[p - 1] <= 3 else 0)  # nt2bit: N -> A
    inner = ts[tpos - 1:tpos - 1 + fl]
    gc = int(((inner == 1) | (inner == 2)).sum()) / fl
    return np.array(frag[:K], np.uint8), np.array(frag[-K:], np.uint8), gc


def make_examples(tseq_ptr, tseq, transcript, tpos, fraglen, seed, cls):
    L, R, G = [], [], []
    for i, (t, p, f) in enumerate(zip(transcript, tpos, fraglen)):
        l, r, g = make_example(np.asarray(tseq[tseq_ptr[t]:tseq_ptr[t + 1]]), int(p), int(f), seed, i, cls)
        L.append(l), R.append(r), G.append(g)
    return np.array(L, np.uint8).reshape(-1, K), np.array(R, np.uint8).reshape(-1, K), np.array(G, np.float64)


def pack(seq):
    """[N, 20] codes -> u64, position 1 in the highest used bits"""
    w = np.zeros(len(seq), np.uint64)
    for j in range(K):
        w = (w << np.uint64(2)) | seq[:, j].astype(np.uint64)
    return w


# ---- SeqBiasModel (bias.jl:184-399) ---------------------------------------------------------------------------------------------------
def contexts(seq, j, order):
    ctx = np.zeros(len(seq), np.int64)
    for l in range(1, order + 1):
        ctx = (ctx << 2) | seq[:, j + l]
    return ctx


def update_param_estimate(ps, seq, ys, j, order):
    ps[j] = 1  # pseudocount
    ctx = contexts(seq, j, order)
    np.add.at(ps[j], (ys.astype(np.int64), seq[:, j].astype(np.int64), ctx), f32(1))
    for i2 in range(2):
        n = 4 ** order
        z = ((ps[j, i2, 0, :n] + ps[j, i2, 1, :n]) + ps[j, i2, 2, :n]) + ps[j, i2, 3, :n]
        ps[j, i2, :, :n] /= z


def update_p(ps, seq, seq_p, j, order):
    if order < 0:
        return
    ctx = contexts(seq, j, order)
    nt = seq[:, j].astype(np.int64)
    seq_p[:, 0, j] = ps[j, 0, nt, ctx]
    seq_p[:, 1, j] = ps[j, 1, nt, ctx]


def ordered_sum(lp):
    n = len(lp)
    v = np.zeros((n + 255) // 256 * 256, np.float64)
    v[:n] = lp
    v = v.reshape(-1, 256)
    s = 128
    while s >= 1:
        v = v[:, :s] + v[:, s:2 * s]
        s //= 2
    return float(np.cumsum(v[:, 0])[-1])


def compute_loss(n_params, seq_p, ys):
    n = len(ys)
    p_fg, p_bg = np.ones(n, f32), np.ones(n, f32)
    for j in range(seq_p.shape[2]):
        p_fg = p_fg * seq_p[:, 1, j]
        p_bg = p_bg * seq_p[:, 0, j]
    with np.errstate(all="ignore"):
        p = p_fg / (p_fg + p_bg)
        q = np.where(ys, p, f32(1) - p).astype(f32)
        ll = ordered_sum(np.log(q.astype(np.float64)))
    return -(2 * ll - n_params * math.log(n))


def added_params(o):
    return 4 ** (1 + o) - (0 if o == 0 else 4 ** o)


def score_candidates(ps, seq, ys, seq_p, orders, n_params):
    """one pass of the loop at bias.jl:357-383 -> losses [20] (+inf where no candidate is allowed); state restored"""
    losses = np.full(K, np.inf)
    for j in range(K):  # 0-based j: the reference's j is j + 1
        if orders[j] < MAXORDER and (j + 1) + orders[j] < K:
            tmp_ps, tmp_p = ps[j].copy(), seq_p[:, :, j].copy()
            orders[j] += 1
            update_param_estimate(ps, seq, ys, j, orders[j])
            update_p(ps, seq, seq_p, j, orders[j])
            losses[j] = compute_loss(n_params + added_params(orders[j]), seq_p, ys)
            orders[j] -= 1
            ps[j], seq_p[:, :, j] = tmp_ps, tmp_p
    return losses


def relative_gap(losses, loss0):
    """how far the round's decision is from flipping: the smallest loss against the runner-up and against loss0"""
    fin = np.sort(losses[np.isfinite(losses)])
    if len(fin) == 0:
        return np.inf
    others = [loss0] + ([fin[1]] if len(fin) > 1 else [])
    return min(abs(fin[0] - x) for x in others) / abs(fin[0])


def seqbias_model(seq, ys):
    """-> dict(orders i32 [20], ps f32 [20, 4, 4096] (fg / bg; 1 where the model never reads), trace [rounds + 1], positions, gap)"""
    n = len(ys)
    ps = np.zeros((K, 2, 4, CTX), f32)
    seq_p = np.ones((n, 2, K), f32)
    orders = np.full(K, -1, np.int64)
    n_params = 0
    loss0 = compute_loss(n_params, seq_p, ys)
    trace, positions, gap = [loss0], [], np.inf
    while True:
        losses = score_candidates(ps, seq, ys, seq_p, orders, n_params)
        gap = min(gap, relative_gap(losses, loss0))
        best_loss, best_j = loss0, -1
        for j in range(K):
            if losses[j] < best_loss:
                best_loss, best_j = losses[j], j
        if best_loss >= loss0:
            break
        orders[best_j] += 1
        update_param_estimate(ps, seq, ys, best_j, orders[best_j])
        update_p(ps, seq, seq_p, best_j, orders[best_j])
        loss0 = best_loss
        n_params += added_params(orders[best_j])
        trace.append(loss0), positions.append(best_j)
    out = np.ones((K, 4, CTX), f32)
    for j in range(K):
        if orders[j] >= 0:
            m = 4 ** orders[j]
            out[j, :, :m] = ps[j, 1, :, :m] / ps[j, 0, :, :m]
    return dict(orders=orders.astype(np.int32), ps=out, trace=np.array(trace), positions=np.array(positions, np.int32), gap=gap)


def candidate_losses(seq, ys, orders_in):
    """polee_bias_train_candidates: the state `orders_in` rebuilt, one round scored -> (losses [20], loss0)"""
    n = len(ys)
    ps = np.zeros((K, 2, 4, CTX), f32)
    seq_p = np.ones((n, 2, K), f32)
    orders = np.asarray(orders_in, np.int64).copy()
    n_params = 0
    for j in range(K):
        if orders[j] >= 0:
            update_param_estimate(ps, seq, ys, j, orders[j])
            update_p(ps, seq, seq_p, j, orders[j])
            n_params += 4 ** (1 + orders[j])
    return score_candidates(ps, seq, ys, seq_p, orders, n_params), compute_loss(n_params, seq_p, ys)


def evaluate(model, seq):
    """evaluate(sb, seq) (bias.jl:402-416) for every row"""
    bias = np.ones(len(seq), f32)
    for j in range(K):
        o = model["orders"][j]
        if o >= 0:
            bias = bias * model["ps"][j, seq[:, j].astype(np.int64), contexts(seq, j, o)]
    return bias


# ---- SimpleHistogramModel (bias.jl:464-514) ---------------------------------------------------------------------------------------------
def histogram_model(xs, ys):
    """xs f32, ys bool -> (expanded bins f32 [100], qs f32 [14])"""
    weights = np.ones(len(xs), f32)
    total_weight = f32(len(xs))  # sum(weights): exact below 2^24
    p = np.argsort(xs, kind="stable")
    xs, ys = xs[p], ys[p]
    numbins = 15
    binsize = f32(total_weight / f32(numbins))
    qs = np.zeros(numbins - 1, f32)
    nextbin, wsum = 1, 0.0
    for x, w in zip(xs, weights):
        wsum += float(w)
        if wsum > float(f32(f32(nextbin) * binsize)):
            qs[nextbin - 1] = x
            nextbin += 1
            if nextbin == numbins:
                break
    bincounts = np.ones((2, numbins), f32)
    idx = np.searchsorted(qs, xs, "left")  # searchsorted(qs, x).start - 1
    np.add.at(bincounts, (ys.astype(np.int64), idx), f32(1))
    sums = [f32(np.cumsum(bincounts[i], dtype=f32)[-1]) for i in range(2)]
    bins = ((bincounts[1] / sums[1]) / (bincounts[0] / sums[0])).astype(f32)
    expanded = np.zeros(100, f32)
    for i in range(1, 101):
        q = (i - 0.5) / 100
        expanded[i - 1] = bins[np.searchsorted(qs.astype(np.float64), q, "left")]
    return expanded, qs


def evaluate_hist(bins, x):
    i = np.clip(np.rint(x * len(bins)).astype(np.int64), 1, len(bins))  # round(Int, .): half to even
    return bins[i - 1]


# ---- accuracy (bias.jl:788-828) ---------------------------------------------------------------------------------------------------------
def accuracy(left_model, right_model, gc_bins, left, right, frag_gc, n_fg):
    bs = (((evaluate(left_model, left) * evaluate(right_model, right)) * evaluate_hist(gc_bins, frag_gc)) * f32(1)).astype(np.float64)
    s = np.sort(bs)
    n = len(s)
    med = s[n // 2] if n % 2 else s[n // 2 - 1] / 2 + s[n // 2] / 2  # Statistics.middle
    bs = bs - med
    acc = int((bs[:n_fg] > 0.0).sum()) + int((bs[n_fg:] <= 0.0).sum())
    return acc / n


def train(left, right, frag_gc, n_fg):
    """BiasModel(...) (bias.jl:677-785) on examples: left / right u8 [N, 20], frag_gc f64 [N], the first n_fg foreground"""
    ys = np.arange(len(frag_gc)) < n_fg
    ml, mr = seqbias_model(left, ys), seqbias_model(right, ys)
    bins, qs = histogram_model(frag_gc.astype(f32), ys)
    return dict(left=ml, right=mr, gc_bins=bins, gc_qs=qs, accuracy=accuracy(ml, mr, bins, left, right, frag_gc, n_fg),
                gap=min(ml["gap"], mr["gap"]))


# ---- planted data ----------------------------------------------------------------------------------------------------------------------
PLANTED_SEED, PLANTED_N = 11, 3001


def planted_examples(seed=PLANTED_SEED, n=PLANTED_N):
    """n foreground + n background examples: background uniform; foreground left end with a skewed base at position 3, position 6
    drawn given positions 7-8, position 19 given position 20, a skewed position 20 (1-based); right end with a skewed position 10;
    frag_gc in 1/200 steps, higher in the foreground.  -> (left, right u8 [2n, 20], frag_gc f64 [2n], n_fg)"""
    rng = np.random.default_rng(seed)
    left, right = rng.integers(0, 4, (2 * n, K)), rng.integers(0, 4, (2 * n, K))
    fg = left[:n]
    fg[:, 2] = rng.choice(4, n, p=[0.55, 0.15, 0.15, 0.15])
    fg[:, 19] = rng.choice(4, n, p=[0.1, 0.4, 0.4, 0.1])
    fg[:, 18] = np.where(rng.random(n) < 0.8, (fg[:, 19] + 1) % 4, fg[:, 18])
    fg[:, 5] = np.where(rng.random(n) < 0.7, np.minimum(fg[:, 6], fg[:, 7]), fg[:, 5])
    right[:n, 9] = rng.choice(4, n, p=[0.1, 0.2, 0.3, 0.4])
    gc = np.concatenate([rng.normal(0.55, 0.1, n), rng.normal(0.45, 0.1, n)])
    gc = np.clip(np.rint(gc * 200), 0, 200) / 200
    return left.astype(np.uint8), right.astype(np.uint8), gc.astype(np.float64), n


@functools.lru_cache(maxsize=None)
def planted_reference():
    """(examples, the restatement's model of them), computed once per process"""
    ex = planted_examples()
    return ex, train(*ex)


def small_examples(n):
    """n + n examples cut from the planted ones (a partial and an exact wave on the device), the foreground's position 3 (left) and
    position 10 (right) made constant so that so few examples still carry a round past the BIC penalty"""
    l, r, g, nf = planted_examples()
    pick = np.concatenate([np.arange(n), nf + np.arange(n)])
    l, r = l[pick].copy(), r[pick].copy()
    l[:n, 2], r[:n, 9] = 0, 3
    return l, r, g[pick], n


def synthetic_transcripts(seed=5, n=40, lo=20, hi=900):
    """transcripts of lo .. hi bases with a few N, the first exactly 20 bases long -> (tseq_ptr i64 [n+1], tseq u8)"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(lo, hi, n)
    lens[0] = 20
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    tseq = rng.integers(0, 4, ptr[-1]).astype(np.uint8)
    tseq[rng.random(ptr[-1]) < 0.01] = 4
    return ptr, tseq


def edge_fragments():
    """fragments on synthetic_transcripts(): both transcript ends (pads on either side), N bases, fraglen 20, the whole 20-base
    transcript 0, and random ones; + three that the Python layer must drop"""
    ptr, tseq = synthetic_transcripts()
    rng = np.random.default_rng(3)
    t, p, f = [0], [1], [20]  # the whole transcript: 5 pads on either side
    for j in range(1, len(ptr) - 1):
        tlen = int(ptr[j + 1] - ptr[j])
        if tlen < 30:
            continue
        fl = int(rng.integers(20, tlen + 1))
        t += [j, j, j, j]
        p += [1, tlen - fl + 1, int(rng.integers(1, tlen - fl + 2)), int(rng.integers(1, tlen - 20 + 2))]
        f += [fl, fl, fl, 20]
    good = len(t)
    t += [1, 2, 3]
    p += [1, 0, int(ptr[4] - ptr[3]) - 18]
    f += [19, 25, 20]  # too short, before the start, over the end
    return ptr, tseq, np.array(t, np.int32), np.array(p, np.int64), np.array(f, np.int32), good
