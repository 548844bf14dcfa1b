"""Plain Python / NumPy restatement (f64, integers) of the fragment model's two kernels (polee_amd/csrc/xbuild.hip, DESIGN.md section
3.18).  Nothing here imports the library.

  fragmentlength            the walk of oracle/xbuild_oracle.c, ported line by line (src/transcripts.jl:273-446)
  estimate                  SimplisticFragModel's counts (src/fragmodel.jl:35-67)
  uniforms, draw, assign    one transcript per row (src/rnaseq_sample.jl:346-373): the draw with a NumPy Philox, and the loop as written
  genomic_to_transcriptomic the fragment's interval on a transcript (src/transcripts.jl:452-538)

Transcripts and fragments are dicts in the layout of polee_xb_transcripts / polee_xb_fragments, mates ordered (m1 the leftmost)."""
import numpy as np

import rng_restatement as R

MAX_FRAG_LEN = 2000
OP_MATCH, OP_INSERT, OP_DELETE, OP_SKIP, OP_SOFT_CLIP = 0, 1, 2, 3, 4
TAG_ASSIGN = 0x66617373  # 'fass'
FLAG_OBSERVED, FLAG_STRAND_MATCH, FLAG_STRAND_MISMATCH = 1, 2, 4
MAX_ENC = 2


def _lists(d, keys):
    return {k: np.asarray(d[k]).tolist() for k in keys}


class Inputs:
    """the arrays as Python lists (element access on NumPy arrays is what makes such loops slow)"""

    def __init__(self, transcripts, fragments):
        self.n, self.m = int(transcripts["n"]), int(fragments["m"])
        t = _lists(transcripts, ("seq", "strand", "exon_ptr", "exon_first", "exon_last"))
        f = _lists(fragments, ("seq", "strand", "m1_left", "m1_right", "m2_left", "m2_right", "m1_is_flag16", "cig1_ptr", "cig2_ptr",
                               "cig_op", "cig_len"))
        self.t_seq, self.t_strand, self.exon_ptr, self.ef, self.el = t["seq"], t["strand"], t["exon_ptr"], t["exon_first"], t["exon_last"]
        self.f_seq, self.f_strand = f["seq"], f["strand"]
        self.m1l, self.m1r, self.m2l, self.m2r = f["m1_left"], f["m1_right"], f["m2_left"], f["m2_right"]
        self.c1, self.c2, self.cop, self.clen = f["cig1_ptr"], f["cig2_ptr"], f["cig_op"], f["cig_len"]
        self.by_seq = {}
        for j in range(self.n):
            self.by_seq.setdefault(self.t_seq[j], []).append(j)

    def exons(self, j):
        a, b = self.exon_ptr[j], self.exon_ptr[j + 1]
        return self.ef[a:b], self.el[a:b]

    def tlen(self, j):
        ef, el = self.exons(j)
        return sum(l - f + 1 for f, l in zip(ef, el))

    def cigar(self, lo, hi, left, right):
        """CigarIter (src/reads.jl:458-492): [(first, last, op)]; an empty range is one match over [left, right]"""
        if hi == lo:
            return [[left, right, OP_MATCH]]
        out, pos = [], left
        for k in range(lo, hi):
            out.append([pos, pos + self.clen[k] - 1, self.cop[k]])
            pos += self.clen[k]
        return out

    def candidates(self, i):
        """transcripts of the fragment's sequence that contain its span (intersect_contains, rnaseq_sample.jl:77-79), ascending"""
        a_first, a_last = self.m1l[i], self.m1r[i]
        if self.m2l[i] > 0 and self.m2r[i] > a_last:
            a_last = self.m2r[i]
        out = []
        for j in self.by_seq.get(self.f_seq[i], ()):
            if self.ef[self.exon_ptr[j]] <= a_first and self.el[self.exon_ptr[j + 1] - 1] >= a_last:
                out.append(j)
        return out


def _exon_compatible(op):
    return op in (OP_MATCH, OP_SOFT_CLIP, OP_INSERT, OP_DELETE)


def _intron_compatible(op):
    return op in (OP_SKIP, OP_SOFT_CLIP)


class _Walk:
    """the exon / intron cursor of next_exonintron (reads.jl:521-537)"""

    def __init__(self, ef, el, idx):
        self.ef, self.el, self.ne = ef, el, len(ef)
        self.idx, self.first, self.last, self.isexon = idx, ef[idx], el[idx], True

    def advance(self):
        if self.isexon:
            if self.idx + 1 < self.ne:
                self.first, self.last = self.el[self.idx] + 1, self.ef[self.idx + 1] - 1
            else:
                self.idx += 1
        else:
            self.idx += 1
            self.first, self.last = self.ef[self.idx], self.el[self.idx]
        self.isexon = not self.isexon


def fragmentlength(I, j, i):
    """-1 incompatible ("nothing"), 0 compatible single-end, > 0 the fragment's length"""
    ef, el = I.exons(j)
    ne = len(ef)
    paired = I.m2l[i] > 0
    a_first, a_last = I.m1l[i], I.m1r[i]
    if paired and I.m2r[i] > a_last:
        a_last = I.m2r[i]
    if a_first < ef[0] or a_last > el[ne - 1]:
        return -1
    first_idx = 0
    for k in range(ne):
        if ef[k] < a_first or (ef[k] == a_first and el[k] <= a_last):
            first_idx = k
        else:
            break
    intronlen = 0
    # the first mate
    cig = I.cigar(I.c1[i], I.c1[i + 1], I.m1l[i], I.m1r[i])
    q = 0
    if q < len(cig) and cig[q][2] == OP_SOFT_CLIP:
        q += 1
    e = _Walk(ef, el, first_idx)
    while e.idx < ne and q < len(cig):
        c = cig[q]
        if e.last < c[0]:
            e.advance()
        elif e.first <= c[1] <= e.last and c[0] >= e.first:
            if e.isexon:
                if not _exon_compatible(c[2]):
                    return -1
            else:
                if not _intron_compatible(c[2]):
                    return -1
                intronlen += e.last - e.first + 1
            q += 1
        elif c[2] == OP_SOFT_CLIP:
            q += 1
        elif c[1] > e.last and c[2] == OP_MATCH:
            if e.isexon and c[1] - e.last <= MAX_ENC:
                c[1] = e.last
            elif not e.isexon and e.last >= c[0] and e.last - c[0] < MAX_ENC:
                c[0] = e.last + 1
            else:
                return -1
        else:
            return -1
    if q < len(cig):
        return -1
    if not paired:
        return 0
    # the second mate: the introns passed after the exon / intron where the first mate's walk ended count as spanned
    cig = I.cigar(I.c2[i], I.c2[i + 1], I.m2l[i], I.m2r[i])
    q = 0
    e2 = _Walk(ef, el, first_idx)
    sup = False
    while e2.idx < ne and q < len(cig):
        c = cig[q]
        if e2.last < c[0]:
            if not e2.isexon and sup:
                intronlen += e2.last - e2.first + 1
            if e.idx < ne and e.first == e2.first and e.last == e2.last:
                sup = True
            e2.advance()
        elif e2.first <= c[1] <= e2.last and c[0] >= e2.first:
            if e2.isexon:
                if not _exon_compatible(c[2]):
                    return -1
            elif not _intron_compatible(c[2]):
                return -1
            q += 1
        elif c[2] == OP_SOFT_CLIP:
            q += 1
        elif c[1] > e2.last and c[2] == OP_MATCH:
            if e2.isexon and c[1] - e2.last <= MAX_ENC:
                c[1] = e2.last
            elif not e2.isexon and e2.last >= c[0] and e2.last - c[0] < MAX_ENC:
                c[0] = e2.last + 1
            else:
                return -1
        else:
            return -1
    if q < len(cig) and cig[q][2] == OP_SOFT_CLIP:
        q += 1
    if q < len(cig):
        return -1
    fraglen = max(I.m1r[i], I.m2r[i]) - min(I.m1l[i], I.m2l[i]) + 1 - intronlen
    return fraglen if fraglen > 0 else -1


def estimate(transcripts, fragments):
    """-> dict(counts i64 [4] = compatible pairs, strand matches, strand mismatches, fragments whose smallest positive length is above
    2000; hist i64 [2000]; min_fraglen i64 [m], 0 = none; pairs: [(i, j, fraglen)] of the compatible pairs)"""
    I = Inputs(transcripts, fragments)
    counts, hist, mins, pairs = np.zeros(4, np.int64), np.zeros(MAX_FRAG_LEN, np.int64), np.zeros(I.m, np.int64), []
    for i in range(I.m):
        mn = 0
        for j in I.candidates(i):
            fl = fragmentlength(I, j, i)
            if fl < 0:
                continue
            pairs.append((i, j, fl))
            counts[0] += 1
            if I.f_strand[i] == I.t_strand[j]:
                counts[1] += 1
            elif I.f_strand[i] in (1, -1):
                counts[2] += 1
            if fl > 0 and (mn == 0 or fl < mn):
                mn = fl
        mins[i] = mn
        if mn > MAX_FRAG_LEN:
            counts[3] += 1
        elif mn > 0:
            hist[mn - 1] += 1
    return dict(counts=counts, hist=hist, min_fraglen=mins, pairs=pairs)


def u01_53(w0, w1):
    """philox_u01_53 (csrc/binomial.hpp): (k + 1/2) 2^-52 with k the 52 bits w0[31:6] w1[31:6]; exact in f64"""
    k = ((np.asarray(w0, np.uint64) >> np.uint64(6)) << np.uint64(26)) | (np.asarray(w1, np.uint64) >> np.uint64(6))
    return (k.astype(np.float64) + 0.5) * (1.0 / 4503599627370496.0)


def uniforms(fragment_ids, seed):
    """the uniform of every fragment: words 0, 1 of the block with counter (low word of i, high word of i, 0, 'fass') under the key seed"""
    i = np.asarray(fragment_ids, np.int64).astype(np.uint64)
    w = R.philox4x32_10(i & R.MASK, i >> np.uint64(32), 0, TAG_ASSIGN, seed)
    return u01_53(w[..., 0], w[..., 1])


def draw(products, u):
    """products: the f32 products xs[j] * nzval of a row, in the row's order; u: its uniform.  -> the position taken: the first with
    zj = product / z_sum > r, r reduced by every zj passed over; the last entry takes what is left."""
    z_sum = 0.0
    for p in products:
        z_sum += float(p)
    r = float(u)
    with np.errstate(all="ignore"):
        for k in range(len(products) - 1):
            zj = float(np.float64(float(products[k])) / np.float64(z_sum))
            if zj > r:
                return k
            r -= zj
    return len(products) - 1


def as_written(products, u):
    """the reference's loop as it is written (rnaseq_sample.jl:359-369): no break, and the condition holds at the last entry"""
    z_sum = 0.0
    for p in products:
        z_sum += float(p)
    r, taken = float(u), -1
    with np.errstate(all="ignore"):
        for k in range(len(products)):
            zj = float(np.float64(float(products[k])) / np.float64(z_sum))
            if zj > r or k == len(products) - 1:
                taken = k
            else:
                r -= zj
    return taken


def g2t_position(I, j, position):
    """genomic_to_transcriptomic(t, position) (transcripts.jl:520-538): 0 = not in an exon"""
    ef, el = I.exons(j)
    i = 0
    for k in range(len(ef)):  # searchsortedlast(exons, Exon(position, position))
        if ef[k] < position or (ef[k] == position and el[k] <= position):
            i = k + 1
        else:
            break
    if i == 0 or el[i - 1] < position:
        return 0
    tpos = 1 + sum(el[k] - ef[k] + 1 for k in range(i - 1)) + position - ef[i - 1]
    if I.t_strand[j] < 0:
        tpos = I.tlen(j) - tpos + 1
    return tpos


def genomic_to_transcriptomic(I, j, i, m1_reverse, fallback_fraglen, tlen=None):
    """genomic_to_transcriptomic(t, rs, alnpr, fraglen_median) (transcripts.jl:452-517) -> (tpos, fraglen); empty: (0, 0)"""
    tlen = I.tlen(j) if tlen is None else tlen
    fraglen = fragmentlength(I, j, i)
    if fraglen < 0:
        return 0, 0
    if fraglen <= 0:
        fraglen = fallback_fraglen
        if fraglen <= 0:
            return 0, 0
    if I.m2l[i] > 0:
        gpos = min(I.m1l[i], I.m2l[i]) if I.t_strand[j] > 0 else max(I.m1r[i], I.m2r[i])
        tpos = g2t_position(I, j, gpos)
    else:
        neg = bool(m1_reverse[i])
        if I.t_strand[j] > 0:
            tpos = g2t_position(I, j, I.m1l[i]) if not neg else g2t_position(I, j, I.m1r[i]) - fraglen
        else:
            tpos = g2t_position(I, j, I.m1l[i]) - fraglen if not neg else g2t_position(I, j, I.m1r[i])
    if tpos <= 0:  # nudge reads that overhang
        fraglen += tpos - 1
        tpos = 1
    if tpos + fraglen - 1 > tlen:
        fraglen = tlen - tpos + 1
    return (tpos, fraglen) if fraglen > 0 else (0, 0)


def assign(transcripts, fragments, x, xs, m1_reverse, seed, mode, fallback_fraglen=150):
    """x: dict(tcolptr, trowval, tnzval, row_fragment) of the rows of X.  mode 0: the draw; mode 1: as written.
    -> dict(transcript i32, tpos i64, fraglen i32, flags u8), one element per row"""
    I = Inputs(transcripts, fragments)
    ptr = np.asarray(x["tcolptr"]).astype(np.int64) - 1
    cols = np.asarray(x["trowval"]).astype(np.int64) - 1
    vals = np.asarray(x["tnzval"], np.float32)
    rf = np.asarray(x["row_fragment"], np.int64)
    rows = len(rf)
    rev = np.zeros(I.m, np.uint8) if m1_reverse is None else np.asarray(m1_reverse, np.uint8)
    out = dict(transcript=np.zeros(rows, np.int32), tpos=np.zeros(rows, np.int64), fraglen=np.zeros(rows, np.int32),
               flags=np.zeros(rows, np.uint8))
    if mode == 0:
        prod = np.asarray(xs, np.float32)[cols] * vals  # f32 products
        us = uniforms(rf, seed)
    for r in range(rows):
        b, e = int(ptr[r]), int(ptr[r + 1])
        k = draw(prod[b:e], us[r]) if mode == 0 else e - b - 1
        i, j = int(rf[r]), int(cols[b + k])
        tpos, fl = genomic_to_transcriptomic(I, j, i, rev, fallback_fraglen)
        fg = FLAG_OBSERVED if I.m2l[i] > 0 else 0
        if fl > 0:
            if I.f_strand[i] == I.t_strand[j]:
                fg |= FLAG_STRAND_MATCH
            elif I.f_strand[i] in (1, -1):
                fg |= FLAG_STRAND_MISMATCH
        out["transcript"][r], out["tpos"][r], out["fraglen"][r], out["flags"][r] = j, tpos, fl, fg
    return out


def make_fragments(frags):
    """[(seq, strand, m1_left, m1_right, m2_left, m2_right, cigar1, cigar2)], a cigar a list of (op, length) -> polee_xb_fragments dict"""
    m = len(frags)
    F = dict(m=m, seq=np.array([f[0] for f in frags], np.int32), strand=np.array([f[1] for f in frags], np.int8),
             m1_left=np.array([f[2] for f in frags], np.int64), m1_right=np.array([f[3] for f in frags], np.int64),
             m2_left=np.array([f[4] for f in frags], np.int64), m2_right=np.array([f[5] for f in frags], np.int64),
             m1_is_flag16=np.zeros(m, np.uint8))
    ops = [op for f in frags for op in f[6]] + [op for f in frags for op in f[7]]
    F["cig1_ptr"] = np.concatenate([[0], np.cumsum([len(f[6]) for f in frags])]).astype(np.int64)
    F["cig2_ptr"] = (F["cig1_ptr"][-1] + np.concatenate([[0], np.cumsum([len(f[7]) for f in frags])])).astype(np.int64)
    F["cig_op"] = np.array([o for o, _ in ops] or [0], np.uint8)
    F["cig_len"] = np.array([l for _, l in ops] or [0], np.int32)
    return F


def overhang_case():
    """Two transcripts of the same two exons (101..200, 301..400: 200 bases), 0 on + and 1 on -, and fragments whose interval overhangs
    a transcript end and is nudged (transcripts.jl:504-512).  -> (T, F, m1_reverse, expected): expected[(i, j)] = (tpos, fraglen)"""
    T = dict(n=2, seq=np.array([0, 0], np.int32), strand=np.array([1, -1], np.int8), exon_ptr=np.array([0, 2, 4], np.int64),
             exon_first=np.array([101, 301, 101, 301], np.int64), exon_last=np.array([200, 400, 200, 400], np.int64))
    S, M = OP_SOFT_CLIP, OP_MATCH
    F = make_fragments([
        (0, 1, 296, 350, 341, 390, [(S, 5), (M, 50)], []),   # 0: soft-clipped past the start of exon 2: its left end is in no exon
        (0, 1, 111, 160, 151, 205, [], [(M, 50), (S, 5)]),   # 1: soft-clipped past the end of exon 1: its right end is in no exon
        (0, 1, 371, 400, 0, 0, [], []),                      # 2: single-end, forward, 30 bases before the transcripts' last base
        (0, -1, 101, 130, 0, 0, [], []),                     # 3: single-end, reverse, 30 bases after the transcripts' first base
        (0, 1, 121, 170, 151, 200, [], [])])                 # 4: inside exon 1, nothing to nudge
    rev = np.array([0, 0, 0, 1, 0], np.uint8)
    F["m1_is_flag16"] = rev.copy()
    expected = {(0, 0): (1, 94), (0, 1): (11, 95), (1, 0): (11, 95), (1, 1): (1, 94), (2, 0): (171, 30), (2, 1): (1, 29),
                (3, 0): (1, 29), (3, 1): (171, 30), (4, 0): (21, 80), (4, 1): (101, 80)}
    return T, F, rev, expected
