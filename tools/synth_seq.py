"""Seeded generator of transcript sequences for `polee fit-tree` (polee_amd/fit_tree.py): gene families whose members are
mutated copies of a founder (substitutions and indels, so relatives share many but not all 32-mers), a few repeat elements
inserted into many unrelated transcripts (k-mers shared by hundreds of transcripts: long value runs in the candidate-edge
step), and a tail of short and N-bearing transcripts.  Feeds the tests and tools/probe/fit_tree_timing.py.

    seqs = make_transcripts(2000, seed=3)            # list of bytes
    write_fasta("t.fa.gz", seqs)                     # ids tx0000001 ..."""
import gzip

import numpy as np

_ACGT = np.frombuffer(b"ACGT", np.uint8)


def _mutate(rng, seq, sub, indel):
    """substitutions at rate `sub`, single-base insertions / deletions at rate `indel`"""
    s = seq.copy()
    hit = rng.random(len(s)) < sub
    s[hit] = _ACGT[rng.integers(0, 4, int(hit.sum()))]
    if indel > 0:
        drop = rng.random(len(s)) < indel / 2
        s = s[~drop]
        pos = np.flatnonzero(rng.random(len(s)) < indel / 2)
        if len(pos):
            s = np.insert(s, pos, _ACGT[rng.integers(0, 4, len(pos))])
    return s


def make_transcripts(n, seed=0, mean_len=2000, family=4.0, repeats=8, repeat_share=0.05, short_share=0.02, n_share=0.02,
                     max_len=None):
    """n transcripts as a list of bytes.  Lengths are log-normal around mean_len (at least 40, at most max_len);
    family: mean family size; repeats: number of 300-base repeat elements, each inserted into ~repeat_share / repeats of the
    transcripts; short_share: transcripts of 0 .. 40 bases; n_share: transcripts with a few N."""
    rng = np.random.default_rng(seed)
    reps = [_ACGT[rng.integers(0, 4, 300)] for _ in range(repeats)]
    out = []
    while len(out) < n:
        ln = int(np.clip(rng.lognormal(np.log(mean_len) - 0.32, 0.8), 40, max_len or 50 * mean_len))
        founder = _ACGT[rng.integers(0, 4, ln)]
        for k in range(min(n - len(out), 1 + int(rng.poisson(family - 1)))):
            s = founder if k == 0 else _mutate(rng, founder, rng.uniform(0.002, 0.03), rng.uniform(0, 0.004))
            if k and rng.random() < 0.3:  # an isoform: a stretch left out
                a = int(rng.integers(0, max(1, len(s) - 40)))
                s = np.concatenate([s[:a], s[a + int(rng.integers(1, max(2, len(s) // 3))):]])
            if repeats and rng.random() < repeat_share:
                r = _mutate(rng, reps[int(rng.integers(repeats))], 0.005, 0.0)
                a = int(rng.integers(0, len(s) + 1))
                s = np.concatenate([s[:a], r, s[a:]])
            out.append(s)
    for i in np.flatnonzero(rng.random(n) < short_share):
        out[i] = out[i][:int(rng.integers(0, 41))]
    for i in np.flatnonzero(rng.random(n) < n_share):
        if len(out[i]):
            s = out[i].copy()
            s[rng.integers(0, len(s), int(rng.integers(1, 4)))] = ord("N")
            out[i] = s
    return [s.tobytes() for s in out]


def write_fasta(filename, seqs, width=70):
    op = gzip.open if str(filename).endswith(".gz") else open
    with op(filename, "wb") as f:
        for i, s in enumerate(seqs):
            f.write(b">tx%07d synthetic\n" % (i + 1))
            for a in range(0, len(s), width):
                f.write(s[a:a + width] + b"\n")
