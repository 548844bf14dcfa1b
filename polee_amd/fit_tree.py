"""`polee fit-tree` (src/main.jl:638-660; src/kmersketch.jl, src/kmercluster.jl): a Polya tree from the transcripts' sequences,
the tree `prep --salmon --ptt-tree` fits on.

    python -m polee_amd.fit_tree transcriptome.fa[.gz] -o tree.h5 [--exclude-transcripts FILE] [--device D] [--host]
                                 [--merge {greedy,rounds}]

Every transcript gets a one-permutation MinHash sketch of its canonical 32-mers (200 bins); transcripts, then subtrees, are
joined greedily by the approximate Jaccard index of their sketches, and what shares no k-mer with anything is joined
Huffman-fashion.  The hash, the bin rule and the order among equal similarities are this project's own, fixed in DESIGN.md
§3.12 (upstream's are Julia's hash and its heap's positions); K = 32, H = 200 and the file format are upstream's.  The
sketches and the candidate edges are computed on the GPU, the merge loop runs on the host; `--host` computes everything on the
host threads and gives the same file.  `--merge rounds` replaces the greedy loop by rounds of mutually-best merges (DESIGN.md
§3.12): another tree, an equally heuristic one, built wholly on the GPU (or, with `--host`, on all host threads); the default
stays `greedy`.  POLEE_BUILD_TIMING=1 prints the builder's phases on stderr.

Upstream's second form (a GFF3 annotation plus a genome) is not built: it reads an undefined variable upstream (`ts_tree`,
main.jl:645) and needs a GFF3 reader this project does not have.
"""
import argparse
import ctypes as C
import gzip
import sys
import time

import numpy as np

from . import _lib as L
from . import h5io
from ._lib import check, ptr

K = 32
H = 200
SKETCH_CHUNK = 8192  # POLEE_KMER_SKETCH_CHUNK: windows per workgroup of the sketch kernel (a longer transcript is split)


def read_fasta(filename, excluded=()):
    """(ids, seqs): identifiers (the header up to the first whitespace, as FASTA.identifier gives it) and sequences (bytes, the
    lines of a record joined) in file order; plain or .gz.  A record whose id is in `excluded` is dropped; an empty record is
    kept; a duplicate identifier is an error."""
    excluded = set(excluded)
    ids, seqs, seen = [], [], set()
    op = gzip.open if str(filename).endswith(".gz") else open
    cur, keep = None, False
    with op(filename, "rb") as f:
        for line in f:
            line = line.rstrip(b"\r\n")
            if line.startswith(b">"):
                if keep:
                    seqs.append(b"".join(cur))
                fields = line[1:].split(None, 1)
                name = fields[0].decode("utf-8", "replace") if fields else ""
                keep = name not in excluded
                cur = []
                if keep:
                    if name in seen:
                        raise ValueError("%s: duplicate sequence identifier %r" % (filename, name))
                    seen.add(name)
                    ids.append(name)
            elif cur is not None:
                if keep and line:
                    cur.append(line.strip())
            elif line.strip():
                raise ValueError("%s: sequence data before the first '>' header" % filename)
        if keep:
            seqs.append(b"".join(cur))
    return ids, seqs


def _concat(seqs):
    seqs = [s.encode("ascii", "replace") if isinstance(s, str) else bytes(s) for s in seqs]
    offsets = np.zeros(len(seqs) + 1, np.int64)
    np.cumsum([len(s) for s in seqs], out=offsets[1:])
    bases = np.frombuffer(b"".join(seqs), np.uint8)
    return offsets, bases


def _context(ctx):
    from .core import default_context
    return ctx or default_context()


def kmer_sketches(seqs, ctx=None, host=False):
    """uint64 [n][200]: the sketches of the sequences (bytes or str), on the GPU (polee_kmer_sketch) or, host=True, on the host
    threads (polee_kmer_sketch_host): bit for bit the same."""
    offsets, bases = _concat(seqs)
    n = len(offsets) - 1
    out = np.zeros((n, H), np.uint64)
    if n == 0:
        return out
    if host:
        check(L.lib().polee_kmer_sketch_host(C.c_int64(n), ptr(offsets, L.i64p), ptr(bases, L.u8p), ptr(out, L.u64p)))
    else:
        ctx = _context(ctx)
        check(L.lib().polee_kmer_sketch(ctx._h, C.c_int64(n), ptr(offsets, L.i64p), ptr(bases, L.u8p), ptr(out, L.u64p)), ctx._h)
    return out


MERGES = ("greedy", "rounds")
STATS = ("rounds", "merges", "left_for_huffman", "reevaluated")


def _merge(merge):
    if merge not in MERGES:
        raise ValueError("merge must be one of %s, not %r" % (", ".join(MERGES), merge))
    return merge == "rounds"


def _stats_out(stats, raw):
    if stats is not None:
        stats.update(zip(STATS, (int(x) for x in raw)))


def kmer_tree(sketches, ctx=None, host=False, merge="greedy", stats=None):
    """(node_parent_idxs, node_js), int32 [2n-1], of n sketches: candidate edges from the GPU (polee_kmer_tree) or, host=True,
    everything on the host (polee_kmer_tree_host): node for node the same tree.  merge="rounds": the merges in rounds of
    mutually-best pairs, on the GPU (polee_kmer_tree_rounds) or on the host threads (polee_kmer_tree_rounds_host) -- another tree
    than the greedy one, the same from both; `stats`, a dict, then receives rounds, merges, left_for_huffman and reevaluated."""
    rounds = _merge(merge)
    sk = np.ascontiguousarray(sketches, np.uint64)
    if sk.ndim != 2 or sk.shape[1] != H or sk.shape[0] < 1:
        raise ValueError("sketches must be uint64 [n][%d] with n >= 1" % H)
    n = sk.shape[0]
    parents, js = np.empty(2 * n - 1, np.int32), np.empty(2 * n - 1, np.int32)
    if rounds:
        raw = np.zeros(4, np.int64)
        if host:
            check(L.lib().polee_kmer_tree_rounds_host(C.c_int64(n), ptr(sk, L.u64p), ptr(parents, L.i32p), ptr(js, L.i32p), ptr(raw, L.i64p)))
        else:
            ctx = _context(ctx)
            check(L.lib().polee_kmer_tree_rounds(ctx._h, C.c_int64(n), ptr(sk, L.u64p), ptr(parents, L.i32p), ptr(js, L.i32p), ptr(raw, L.i64p)),
                  ctx._h)
        _stats_out(stats, raw)
        return parents, js
    if host:
        check(L.lib().polee_kmer_tree_host(C.c_int64(n), ptr(sk, L.u64p), ptr(parents, L.i32p), ptr(js, L.i32p)))
    else:
        ctx = _context(ctx)
        check(L.lib().polee_kmer_tree(ctx._h, C.c_int64(n), ptr(sk, L.u64p), ptr(parents, L.i32p), ptr(js, L.i32p)), ctx._h)
    return parents, js


def kmer_candidate_edges(sketches, ctx=None, host=False):
    """the candidate edges the tree starts from, as arrays (u, v, mat, empt) sorted by (u, v) (include/polee_hip_debug.h)"""
    sk = np.ascontiguousarray(sketches, np.uint64)
    n = sk.shape[0]
    h = None if host else _context(ctx)._h
    count = C.c_int64()
    check(L.lib().polee_debug_kmer_edges_count(h, C.c_int64(n), ptr(sk, L.u64p), C.byref(count)), h)
    out = [np.zeros(count.value, np.uint32) for _ in range(4)]
    check(L.lib().polee_debug_kmer_edges_fill(h, C.c_int64(n), ptr(sk, L.u64p), C.c_int64(count.value),
                                              *[ptr(a, L.u32p) for a in out]), h)
    return tuple(out)


def kmer_round_select(num_nodes, u, v, key, ctx=None, host=False):
    """one best-and-select step of the rounds merge on caller-supplied edges (1-based u < v) and 64-bit keys
    (polee_debug_kmer_round_select): (merged uint8 [E], order int32 [E])"""
    u, v, key = np.ascontiguousarray(u, np.uint32), np.ascontiguousarray(v, np.uint32), np.ascontiguousarray(key, np.uint64)
    if not (u.shape == v.shape == key.shape and u.ndim == 1):
        raise ValueError("u, v and key must be one-dimensional and of one length")
    merged, order = np.zeros(len(u), np.uint8), np.zeros(len(u), np.int32)
    h = None if host else _context(ctx)._h
    check(L.lib().polee_debug_kmer_round_select(h, C.c_int64(num_nodes), C.c_int64(len(u)), ptr(u, L.u32p), ptr(v, L.u32p), ptr(key, L.u64p),
                                                ptr(merged, L.u8p), ptr(order, L.i32p)), h)
    return merged, order


def build_polya_tree_transformation(seqs, ctx=None, host=False, merge="greedy", stats=None):
    """sequences -> (node_parent_idxs, node_js) (build_polya_tree_transformation, kmercluster.jl:96-262).  On the GPU the
    sketches stay on the device between the two steps (polee_fit_tree; merge="rounds": polee_fit_tree_rounds, and `stats` as in
    kmer_tree)."""
    rounds = _merge(merge)
    if len(seqs) < 1:
        raise ValueError("no sequences")
    if host:
        return kmer_tree(kmer_sketches(seqs, host=True), host=True, merge=merge, stats=stats)
    offsets, bases = _concat(seqs)
    n = len(offsets) - 1
    ctx = _context(ctx)
    parents, js = np.empty(2 * n - 1, np.int32), np.empty(2 * n - 1, np.int32)
    if rounds:
        raw = np.zeros(4, np.int64)
        check(L.lib().polee_fit_tree_rounds(ctx._h, C.c_int64(n), ptr(offsets, L.i64p), ptr(bases, L.u8p), ptr(parents, L.i32p), ptr(js, L.i32p),
                                            ptr(raw, L.i64p)), ctx._h)
        _stats_out(stats, raw)
        return parents, js
    check(L.lib().polee_fit_tree(ctx._h, C.c_int64(n), ptr(offsets, L.i64p), ptr(bases, L.u8p), ptr(parents, L.i32p), ptr(js, L.i32p)), ctx._h)
    return parents, js


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m polee_amd.fit_tree", description=__doc__.split("\n\n")[0])
    ap.add_argument("sequences", metavar="transcriptome.fa[.gz]")
    ap.add_argument("genome", nargs="?", default=None, help=argparse.SUPPRESS)
    ap.add_argument("-o", "--output", default="ptt-tree.h5", metavar="tree.h5")
    ap.add_argument("--exclude-transcripts", default=None, metavar="FILE", help="transcript ids to leave out, one per line")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--host", action="store_true", help="sketches and candidate edges on the host threads too: no GPU needed")
    ap.add_argument("--merge", choices=MERGES, default="greedy",
                    help="greedy: one best pair at a time (the default); rounds: every round merges all mutually-best pairs, on the GPU")
    a = ap.parse_args(argv)
    if a.genome is not None or a.sequences.lower().endswith((".gff", ".gff3", ".gff.gz", ".gff3.gz")):
        sys.stderr.write("fit-tree from a GFF3 annotation and a genome is not supported: upstream's form reads an undefined variable "
                         "(ts_tree, main.jl:645) and this project has no GFF3 reader.  Give the transcript sequences as FASTA.\n")
        return 2
    excluded = ()
    if a.exclude_transcripts:
        with open(a.exclude_transcripts) as f:
            excluded = [line.strip() for line in f if line.strip()]
    t0 = time.time()
    ids, seqs = read_fasta(a.sequences, excluded)
    t_read = time.time() - t0
    if not ids:
        sys.stderr.write("%s holds no sequences\n" % a.sequences)
        return 1
    t0 = time.time()
    stats = {}
    if a.host:
        parents, js = build_polya_tree_transformation(seqs, host=True, merge=a.merge, stats=stats)
    else:
        from .core import Context
        parents, js = build_polya_tree_transformation(seqs, ctx=Context(a.device), merge=a.merge, stats=stats)
    t_tree = time.time() - t0
    t0 = time.time()
    h5io.write_transformation(a.output, parents, js, ids, " ".join(argv if argv is not None else sys.argv[1:]))
    how = "greedy merges" if a.merge == "greedy" else "merges in %d rounds" % stats["rounds"]
    print("wrote %s (n=%d, %d bases): read %.2f s, sketches and tree (%s, %s) %.2f s, write %.2f s"
          % (a.output, len(ids), sum(len(s) for s in seqs), t_read, "host" if a.host else "device", how, t_tree, time.time() - t0))
    return 0


if __name__ == "__main__":
    sys.exit(main())
