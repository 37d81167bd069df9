"""Reverse Cuthill-McKee stated on the CPU, in the two forms include/smm_hip.h ("a BANDWIDTH-REDUCING ORDERING") speaks of.

A helper, not a test: this is the definition csrc/smm_rcm.hip is compared with.  Everything is integer work, so the comparison is exact.
  graph      vertices i != j are adjacent when (i, j) or (j, i) is stored (explicit zeros count), the diagonal is ignored;
             deg(v) = number of distinct neighbours, key(v) = (deg(v), v) compared lexicographically.
  loop       while unnumbered vertices remain: s = the unnumbered vertex of smallest key; r = the George-Liu root found from s; the
             component of r is numbered by Cuthill-McKee from r and appended to the order.  With `reverse` the whole order is reversed.
  rcm_queue  numbers a component with the classical queue: pop u, append its still unnumbered neighbours in ascending key order.
  rcm_levels numbers it level by level: a new vertex takes parent = the smallest rank among its neighbours in the current level, the new
             level is numbered in ascending (parent, deg, index).  The two give the same order (tests/test_rcm_cpu.py asserts it).
perm[i] is the row that becomes row i: the convention of smm_hip_csr_permute_create."""
import numpy as np


def adjacency(csr):
    """(astart, apos): per vertex its distinct neighbours, ascending, as CSR arrays; the union of the pattern and its transpose
    without the diagonal"""
    start, pos = np.asarray(csr[0], dtype=np.int64), np.asarray(csr[1], dtype=np.int64)
    n = len(start) - 1
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(start))
    cols = pos[:start[-1]]
    off = rows != cols
    u = np.concatenate([rows[off], cols[off]])
    v = np.concatenate([cols[off], rows[off]])
    pairs = np.unique(u * max(n, 1) + v)
    astart = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(pairs // max(n, 1), minlength=n), out=astart[1:])
    return astart, pairs % max(n, 1)


def bfs_levels(astart, apos, root, numbered):
    """the levels (lists of vertices, in no particular order) of a breadth-first search from `root` over unnumbered vertices"""
    seen = {root}
    levels = [[root]]
    while True:
        new = []
        for u in levels[-1]:
            for w in apos[astart[u]:astart[u + 1]]:
                w = int(w)
                if w not in seen and not numbered[w]:
                    seen.add(w)
                    new.append(w)
        if not new:
            return levels
        levels.append(new)


def find_root(astart, apos, deg, s, numbered):
    """George-Liu from s: (root, its BFS levels).  v = the vertex of smallest key in the last level; while v's BFS is deeper, v replaces
    the root."""
    r, levels = s, bfs_levels(astart, apos, s, numbered)
    while True:
        v = min(levels[-1], key=lambda w: (deg[w], w))
        other = bfs_levels(astart, apos, v, numbered)
        if len(other) <= len(levels):
            return r, levels
        r, levels = v, other


def number_queue(astart, apos, deg, r, numbered):
    """classical Cuthill-McKee: the component of r in queue order"""
    queue = [r]
    numbered[r] = True
    head = 0
    while head < len(queue):
        u = queue[head]
        head += 1
        fresh = sorted((int(w) for w in apos[astart[u]:astart[u + 1]] if not numbered[w]), key=lambda w: (deg[w], w))
        for w in fresh:
            numbered[w] = True
        queue.extend(fresh)
    return queue


def number_levels(astart, apos, deg, r, numbered, base):
    """the level-synchronous form: `base` is the rank r receives"""
    rank = {r: base}
    order = [r]
    level = [r]
    numbered[r] = True
    while True:
        parent = {}
        for u in level:
            for w in apos[astart[u]:astart[u + 1]]:
                w = int(w)
                if not numbered[w]:
                    parent[w] = min(parent.get(w, rank[u]), rank[u])
        if not parent:
            return order
        level = sorted(parent, key=lambda w: (parent[w], deg[w], w))
        for w in level:
            rank[w] = base + len(order)
            order.append(w)
            numbered[w] = True


def _rcm(csr, reverse, form):
    n = len(csr[0]) - 1
    astart, apos = adjacency(csr)
    deg = np.diff(astart)
    by_key = np.lexsort((np.arange(n), deg))  # the vertices in ascending key order
    numbered = np.zeros(n, dtype=bool)
    iso = int(np.count_nonzero(deg == 0))
    order = [int(v) for v in by_key[:iso]]  # the isolated vertices, in index order
    numbered[by_key[:iso]] = True
    components, depth = iso, (1 if iso else 0)
    for s in by_key[iso:]:
        s = int(s)
        if numbered[s]:
            continue
        r, levels = find_root(astart, apos, deg, s, numbered)
        components += 1
        depth = max(depth, len(levels))
        order.extend(number_queue(astart, apos, deg, r, numbered) if form == "queue" else number_levels(astart, apos, deg, r, numbered, len(order)))
    perm = np.array(order[::-1] if reverse else order, dtype=np.int32).reshape(n)
    return perm, {"components": components, "levels": depth, "bandwidth_before": bandwidth(csr)[0], "bandwidth_after": bandwidth(csr, perm)[0]}


def rcm_queue(csr, reverse=True):
    """(perm, info) by the queue form"""
    return _rcm(csr, reverse, "queue")


def rcm_levels(csr, reverse=True):
    """(perm, info) by the level-synchronous form"""
    return _rcm(csr, reverse, "levels")


def bandwidth(csr, perm=None):
    """(max |i - j|, number of distinct j - i) over the stored entries of csr, or of P csr Pᵀ when perm is given (the matrix is not built)"""
    start, pos = np.asarray(csr[0], dtype=np.int64), np.asarray(csr[1], dtype=np.int64)
    n = len(start) - 1
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(start))
    cols = pos[:start[-1]]
    if perm is not None:
        inv = np.empty(n, dtype=np.int64)
        inv[np.asarray(perm, dtype=np.int64)] = np.arange(n)
        rows, cols = inv[rows], inv[cols]
    if len(rows) == 0:
        return 0, 0
    return int(np.abs(cols - rows).max()), int(len(np.unique(cols - rows)))


def components_of(csr):
    """label[v]: the number of v's connected component (numbered by smallest vertex)"""
    astart, apos = adjacency(csr)
    n = len(astart) - 1
    label = np.full(n, -1, dtype=np.int64)
    count = 0
    for v in range(n):
        if label[v] >= 0:
            continue
        stack = [v]
        label[v] = count
        while stack:
            u = stack.pop()
            for w in apos[astart[u]:astart[u + 1]]:
                if label[w] < 0:
                    label[w] = count
                    stack.append(int(w))
        count += 1
    return label
