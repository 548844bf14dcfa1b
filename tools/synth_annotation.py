"""A generated annotation for the splicing features (polee_amd/splicing.py): genes of 1 to 12 isoforms drawn from a shared pool of exons
with skipped exons, alternatives of which an isoform takes one, shifted splice sites, retained introns and shifted or dropped ends, on 3
sequences and both strands.  generate(num_transcripts, seed) -> the arrays of polee_xb_transcripts plus gene_of (1-based) and
transcript ids; transcripts come in a shuffled order, so that a gene's isoforms are not neighbours.

    python tools/synth_annotation.py -n 200000 --seed 1 -o transcripts.npz   # (+ transcripts.ids.txt; --gene-pattern '^(G\\d+)\\.')"""
import argparse

import numpy as np

SHIFTS = (0, 0, 0, 12, 27, -15)
END_SHIFTS = (0, 0, 0, 40, 260, 700)


def _isoform(rng, pool, alternatives):
    """one isoform of a gene: a list of (first, last), ascending and disjoint"""
    k = len(pool)
    keep = np.ones(k, bool)
    keep[1:k - 1] = rng.random(max(0, k - 2)) > 0.25  # skipped exons
    for group in alternatives:                         # exactly one of a group of alternatives
        keep[list(group)] = False
        keep[group[rng.integers(len(group))]] = True
    if k > 3 and rng.random() < 0.15:                  # another first or last exon
        keep[0 if rng.random() < 0.5 else k - 1] = False
    exons = [list(pool[i]) for i in range(k) if keep[i]]
    for j in range(len(exons)):                        # shifted splice sites
        if j > 0 and rng.random() < 0.15:
            exons[j][0] += SHIFTS[rng.integers(len(SHIFTS))]
        if j + 1 < len(exons) and rng.random() < 0.15:
            exons[j][1] += SHIFTS[rng.integers(len(SHIFTS))]
    if len(exons) > 2 and rng.random() < 0.12:         # a retained intron
        j = int(rng.integers(len(exons) - 1))
        exons[j:j + 2] = [[exons[j][0], exons[j + 1][1]]]
    exons[0][0] -= END_SHIFTS[rng.integers(len(END_SHIFTS))]
    exons[-1][1] += END_SHIFTS[rng.integers(len(END_SHIFTS))]
    return [(a, b) for a, b in exons]


def generate(num_transcripts, seed=1):
    rng = np.random.default_rng(seed)
    cursor = [2000, 2000, 2000]
    transcripts, genes, g = [], [], 0
    while len(transcripts) < num_transcripts:
        g += 1
        seq, strand = int(rng.integers(3)), int(rng.choice((-1, 1)))
        k = int(rng.integers(3, 13))
        pos, pool = cursor[seq], []
        for _ in range(k):
            length = int(rng.integers(80, 400))
            pool.append((pos, pos + length - 1))
            pos += length + int(rng.integers(300, 2500))
        alternatives = []
        if k >= 5 and rng.random() < 0.4:  # two or three alternatives between fixed neighbours, sometimes overlapping ones
            at = int(rng.integers(1, k - 3))
            size = 2 if rng.random() < 0.7 else 3
            alternatives.append(tuple(range(at, at + size)))
            if size == 3 and rng.random() < 0.4:  # two of the three overlap: they merge into one union, and two unions remain
                pool[at + 1] = (pool[at][0] + 30, pool[at][1] + 30)
        cursor[seq] = pos + 3000
        for i in range(min(int(rng.integers(1, 13)), num_transcripts - len(transcripts))):
            transcripts.append((seq, strand, _isoform(rng, pool, alternatives)))
            genes.append(g)
    order = rng.permutation(len(transcripts))
    transcripts, genes = [transcripts[i] for i in order], np.asarray(genes, np.int64)[order]
    ids, count = [], {}
    for gene in genes:
        count[gene] = count.get(gene, 0) + 1
        ids.append("G%d.%d" % (gene, count[gene]))
    # gene numbers in order of first appearance, as regression.gene_map numbers them from the ids
    first_seen = {}
    for gene in genes:
        first_seen.setdefault(int(gene), len(first_seen) + 1)
    ptr = np.concatenate([[0], np.cumsum([len(t[2]) for t in transcripts])]).astype(np.int64)
    ex = np.array([e for t in transcripts for e in t[2]], np.int64).reshape(-1, 2)
    return dict(n=len(transcripts), seq=np.array([t[0] for t in transcripts], np.int32), strand=np.array([t[1] for t in transcripts], np.int8),
                exon_ptr=ptr, exon_first=np.ascontiguousarray(ex[:, 0]), exon_last=np.ascontiguousarray(ex[:, 1]),
                gene_of=np.array([first_seen[int(gene)] for gene in genes], np.int32), transcript_ids=ids)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("-n", "--num-transcripts", type=int, default=2000)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("-o", "--output", default="transcripts.npz")
    a = ap.parse_args(argv)
    T = generate(a.num_transcripts, a.seed)
    np.savez(a.output, t_seq=T["seq"], t_strand=T["strand"], exon_ptr=T["exon_ptr"], exon_first=T["exon_first"], exon_last=T["exon_last"])
    ids_path = a.output[:-4] + ".ids.txt" if a.output.endswith(".npz") else a.output + ".ids.txt"
    with open(ids_path, "w") as f:
        f.write("\n".join(T["transcript_ids"]) + "\n")
    print("%d transcripts, %d exons, %d genes -> %s, %s" % (T["n"], len(T["exon_first"]), int(T["gene_of"].max()), a.output, ids_path))


if __name__ == "__main__":
    main()
