"""Plain-Python model of the first half of `local` (seed index, read mapping, insert size, collector), written from the
description of what the reference computes, as the yardstick of mhx_local_index / _map / _insert_size / _collect.

Sequences are sequences of ints 0..3 (A, C, G, T).  Nothing here is fast; the cases are a few thousand reads.
"""
import math

DUP = None  # value of a seed that occurs twice in the index: never used
MAX_LOCAL_RANGE = 650
BATCH = 1 << 18


def lround(x):
    """C's lround for x >= 0: halves go up"""
    f = math.floor(x)
    return int(f) + (1 if x - f >= 0.5 else 0)


def _windows(seq, k):
    """-> (position of the window's first base, canonical key, the reverse complement is the smaller) for every window"""
    n = len(seq)
    if n < k:
        return
    mask = (1 << (2 * k)) - 1
    f = r = 0
    for i in range(n):
        b = int(seq[i])
        f = ((f << 2) | b) & mask
        r = (r >> 2) | ((3 - b) << (2 * (k - 1)))
        if i >= k - 1:
            yield i - k + 1, (r if r < f else f), (1 if r < f else 0)


def keep_contigs(contigs, min_len=200, loop_flag=2):
    """contigs: [(bases, flag)] as in the file -> the bases of the kept ones (long enough, no loop), ids = positions in the result"""
    return [c for c, flag in contigs if len(c) >= min_len and not (flag & loop_flag)]


def build_index(contigs, seed_kmer, sparsity):
    """-> {canonical key: (contig, offset, strand) or DUP}, number of seed slots"""
    index = {}
    slots = 0
    for cid, c in enumerate(contigs):
        for j, key, rc in _windows(c, seed_kmer):
            if j % sparsity:
                continue
            slots += 1
            index[key] = DUP if key in index else (cid, j, rc)
    return index, slots


def _matches(read, contig, cfrom, cto, qfrom, qto, strand):
    n = 0
    for t in range(qto - qfrom + 1):
        c = contig[cfrom + t] if strand == 0 else 3 - contig[cto - t]
        n += int(read[qfrom + t]) == int(c)
    return n


INVALID = dict(contig_id=0, contig_from=0, contig_to=0, query_from=0, query_to=0, mismatch=0, strand=0, valid=0)


def try_map(read, index, contigs, seed_kmer, min_mapping_len, similarity):
    """-> the record of the read (a dict with the fields of mhx_local_record)"""
    n = len(read)
    if n < seed_kmer or n < 50:
        return dict(INVALID)
    cands = set()
    for p, key, qrc in _windows(read, seed_kmer):
        hit = index.get(key, DUP)
        if hit is DUP:
            continue
        cid, off, crc = hit
        strand = crc ^ qrc
        clen = len(contigs[cid])
        # where the read's first and last base fall on the contig, were it not clipped
        if strand == 0:
            lo, hi = off - p, off - p + n - 1
        else:
            lo, hi = off + seed_kmer - 1 + p - (n - 1), off + seed_kmer - 1 + p
        cfrom, cto = max(lo, 0), min(hi, clen - 1)
        span = cto - cfrom + 1
        if span < n and span < min_mapping_len:
            continue
        if strand == 0:
            qfrom, qto = cfrom - lo, cto - lo
        else:
            qfrom, qto = hi - cto, hi - cfrom
        cands.add((cid, cfrom, cto, qfrom, qto, strand))
    best, best_m, n_best = None, 0, 0
    for c in cands:
        cid, cfrom, cto, qfrom, qto, strand = c
        m = _matches(read, contigs[cid], cfrom, cto, qfrom, qto, strand)
        if m < lround(similarity * (qto - qfrom + 1)) or m <= 0:
            continue
        if m > best_m:
            best, best_m, n_best = c, m, 1
        elif m == best_m:
            n_best += 1
    if best is None or n_best != 1:
        return dict(INVALID)
    cid, cfrom, cto, qfrom, qto, strand = best
    return dict(contig_id=cid, contig_from=cfrom, contig_to=cto, query_from=qfrom, query_to=qto, mismatch=qto - qfrom + 1 - best_m,
                strand=strand, valid=1)


def map_reads(reads, index, contigs, seed_kmer=31, min_mapping_len=75, similarity=0.8):
    return [try_map(r, index, contigs, seed_kmer, min_mapping_len, similarity) for r in reads]


def insert_size(recs, read_len, begin, end, max_read_len, paired):
    """-> (mean, sd, local range) of the library [begin, end)"""
    mean = sd = 0.0
    if paired:
        hist = {}
        size = 0
        done = begin
        while size < BATCH and done < end:
            start, done = done, min(done + BATCH, end)
            for i in range(start, done - 1, 2):
                a, b = recs[i], recs[i + 1]
                if not (a["valid"] and b["valid"]) or a["contig_id"] != b["contig_id"] or a["strand"] == b["strand"]:
                    continue
                fwd, rev, rl = (a, b, read_len[i + 1]) if a["strand"] == 0 else (b, a, read_len[i])
                # from the forward mate's first base to the reverse mate's, both extended to their unclipped ends
                v = rev["contig_to"] + rl - rev["query_to"] - (fwd["contig_from"] - fwd["query_from"])
                if v >= read_len[i] and v >= read_len[i + 1]:
                    hist[v] = hist.get(v, 0) + 1
                    size += 1
        # trim whole values from either side while they fit into half a per cent each
        trim = int(size * 0.01 / 2 + 0.5)
        gone = []
        s = 0
        for v in sorted(hist):
            if s + hist[v] > trim:
                break
            s += hist[v]
            gone.append(v)
        size -= s
        s = 0
        for v in sorted(hist, reverse=True):
            if s + hist[v] > trim:
                break
            s += hist[v]
            gone.append(v)
        size -= s
        for v in set(gone):
            del hist[v]
        if size:
            mean = float(sum(v * n for v, n in hist.items()) // size)  # an integer quotient
            s1 = s2 = 0.0
            for v in sorted(hist):
                s1 += 1.0 * v * hist[v]
                s2 += 1.0 * v * v * hist[v]
            sd = math.sqrt(s2 / size - (s1 / size) * (s1 / size))
        else:
            sd = float("nan")
    rng = max_read_len - 1
    if paired and mean >= max_read_len:
        rng = int(min(2 * mean, mean + 3 * sd))
    return mean, sd, min(rng, MAX_LOCAL_RANGE)


def _encode(offset, is_mate, mismatch, strand, read_id):
    assert offset < (1 << 14) and read_id < (1 << 44)
    return ((((offset << 1 | is_mate) << 4 | min(mismatch, 15)) << 1 | strand) << 44) | read_id


def _single(groups, r, clen, rlen, rng, read_id):
    if r["contig_to"] < rng and r["query_from"] != 0 and r["query_to"] == rlen - 1:
        groups.setdefault((r["contig_id"], 0), []).append(_encode(r["contig_to"], 0, r["mismatch"], r["strand"], read_id))
        return 1
    if r["contig_from"] + rng >= clen and r["query_to"] < rlen - 1 and r["query_from"] == 0:
        groups.setdefault((r["contig_id"], 1), []).append(_encode(clen - 1 - r["contig_from"], 0, r["mismatch"], r["strand"], read_id))
        return 1
    return 0


def _mate(groups, r, other, clen, rng, mate_id):
    if other["valid"] and other["contig_id"] == r["contig_id"]:
        return 0
    if r["contig_to"] < rng and r["strand"] == 1:
        groups.setdefault((r["contig_id"], 0), []).append(_encode(r["contig_to"], 1, r["mismatch"], r["strand"], mate_id))
        return 1
    if r["contig_from"] + rng >= clen and r["strand"] == 0:
        groups.setdefault((r["contig_id"], 1), []).append(_encode(clen - 1 - r["contig_from"], 1, r["mismatch"], r["strand"], mate_id))
        return 1
    return 0


def collect(recs, read_len, contigs, libs):
    """libs: [(begin, end, paired, local range)] -> (aligned per library, added per library, items, offsets)"""
    groups = {}
    aligned, added = [], []
    for begin, end, paired, rng in libs:
        m = a = 0
        if paired:
            for i in range(begin, end - 1, 2):
                for x, y in ((i, i + 1), (i + 1, i)):
                    r = recs[x]
                    if r["valid"]:
                        m += 1
                        clen = len(contigs[r["contig_id"]])
                        a += _single(groups, r, clen, read_len[x], rng, x)
                        a += _mate(groups, r, recs[y], clen, rng, y)
        else:
            for i in range(begin, end):
                r = recs[i]
                if r["valid"]:
                    m += 1
                    a += _single(groups, r, len(contigs[r["contig_id"]]), read_len[i], rng, i)
        aligned.append(m)
        added.append(a)
    items, offsets = [], [0]
    for cid in range(len(contigs)):
        for end in (0, 1):
            items += sorted(groups.get((cid, end), []))
            offsets.append(len(items))
    return aligned, added, items, offsets
