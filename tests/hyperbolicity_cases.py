"""Truth and inputs of the hyperbolicity tests: a numpy restatement of what ``hm_gromov_delta_*`` documents,
a brute-force four-point delta, graph builders and an all-pairs BFS on the host.  Nothing here touches the library."""
import numpy as np

TILE, KCHUNK = 128, 32                      # hm_gromov_plan.h: the tile edge and the k chunk the kernel ships


def upper(D):
    """D(i, j) := d[min(i, j), max(i, j)]: the matrix the kernel reads."""
    D = np.asarray(D)
    return np.triu(D) + np.triu(D, 1).T


def _per_base(P, neg):
    """(value matrix over i <= j, inner maxima) of the product matrix P: M(i, j) = max_k min(P(i, k), P(k, j))."""
    n = P.shape[0]
    M = np.empty_like(P)
    for i in range(n):
        M[i] = np.minimum(P[i][:, None], P).max(axis=0)
    V = M - P
    V[np.tril_indices(n, -1)] = neg
    return V, M


def _truth(P_of, D, bases, neg):
    values, witnesses = [], []
    for w in bases:
        P = P_of(D, int(w))
        V, M = _per_base(P, neg)
        i, j = np.unravel_index(int(np.argmax(V)), V.shape)          # first maximum in row-major order: smallest i, then smallest j
        k = int(np.argmax(np.minimum(P[i], P[:, j]) == M[i, j]))       # the smallest k that attains the inner maximum
        values.append(V[i, j])
        witnesses.append((int(i), int(j), k))
    return np.array(values), np.array(witnesses, dtype=np.int32).reshape(-1, 3)


def truth_i16(D, bases):
    """(int32 [n_base] 2 delta_w, int32 [n_base, 3] witnesses) of an integer distance matrix."""
    D = upper(D).astype(np.int64)
    v, wit = _truth(lambda D, w: D[:, w][:, None] + D[:, w][None, :] - D, D, bases, np.iinfo(np.int64).min)
    return v.astype(np.int32), wit


def products_f32(D, w):
    """A_w = 0.5f * ((D(i, w) + D(j, w)) - D(i, j)) + 0.0f, every step rounded to float32."""
    col = D[:, w]
    s = (col[:, None] + col[None, :]).astype(np.float32)
    s = (s - D).astype(np.float32)
    return ((np.float32(0.5) * s).astype(np.float32) + np.float32(0.0)).astype(np.float32)


def truth_f32(D, bases):
    """(float32 [n_base] delta_w, witnesses) of a float32 distance matrix, in the kernel's evaluation order."""
    D = upper(np.asarray(D, dtype=np.float32))
    v, wit = _truth(products_f32, D, bases, -np.inf)
    return v.astype(np.float32), wit


def four_point_twice_delta(D):
    """max over all quadruples of S1 - S2, the two largest of the three pair sums: twice the four-point delta."""
    D = np.asarray(D).astype(np.int64)
    n = D.shape[0]
    best = 0
    for x in range(n):
        a = D[x][:, None, None] + D[None, :, :]                     # d(x, y) + d(z, w) as [y, z, w]
        b = D[x][None, :, None] + D[:, None, :]                     # d(x, z) + d(y, w)
        c = D[x][None, None, :] + D[:, :, None]                     # d(x, w) + d(y, z)
        s = np.sort(np.stack([a, b, c]), axis=0)
        best = max(best, int((s[2] - s[1]).max()))
    return best


# ---- graphs: (n, edges int64 [E, 2]) -----------------------------------------------------------------------------------------
def tree(n):
    return n, np.array([((k - 1) // 2, k) for k in range(1, n)], dtype=np.int64).reshape(-1, 2)


def cycle(n):
    return n, np.array([(k, (k + 1) % n) for k in range(n)], dtype=np.int64)


def grid(rows, cols):
    e = [(r * cols + c, r * cols + c + 1) for r in range(rows) for c in range(cols - 1)]
    e += [(r * cols + c, (r + 1) * cols + c) for r in range(rows - 1) for c in range(cols)]
    return rows * cols, np.array(e, dtype=np.int64)


def tree_with_chord(n, a, b):
    _, e = tree(n)
    return n, np.concatenate([e, np.array([[a, b]], dtype=np.int64)])


def star(n):
    return n, np.array([(0, k) for k in range(1, n)], dtype=np.int64).reshape(-1, 2)


def random_connected(n, extra, seed):
    """A random spanning tree plus ``extra`` random chords."""
    rs = np.random.RandomState(seed)
    e = [(int(rs.randint(0, k)), k) for k in range(1, n)]
    while n >= 2 and len(e) < n - 1 + extra:
        a, b = (int(v) for v in rs.randint(0, n, 2))
        if a != b:
            e.append((a, b))
    return n, np.array(e, dtype=np.int64).reshape(-1, 2)


def bfs_all_pairs(n, edges):
    """int16 [n, n] shortest-path lengths, -1 where no path exists."""
    nb = [[] for _ in range(n)]
    for a, b in np.asarray(edges).reshape(-1, 2):
        nb[int(a)].append(int(b))
        nb[int(b)].append(int(a))
    D = np.full((n, n), -1, dtype=np.int16)
    for s in range(n):
        D[s, s] = 0
        front, level = [s], 0
        while front:
            level += 1
            nxt = []
            for u in front:
                for v in nb[u]:
                    if D[s, v] < 0:
                        D[s, v] = level
                        nxt.append(v)
            front = nxt
    return D


GRAPHS = {                                   # name -> (builder, twice the four-point delta; None: only compared with brute force)
    "tree15": (lambda: tree(15), 0),
    "c8": (lambda: cycle(8), 4),
    "c9": (lambda: cycle(9), 3),
    "c12": (lambda: cycle(12), 6),
    "grid4x5": (lambda: grid(4, 5), 6),
    "tree15_chord": (lambda: tree_with_chord(15, 7, 14), 2),
    "random24": (lambda: random_connected(24, 10, 3), None),
}


def cycle_metric(n, circumference=65534, seed=0):
    """int16 [n, n]: distances between n distinct positions on a cycle of the given circumference (D up to 32767)."""
    pos = np.sort(np.random.RandomState(seed).choice(circumference, size=n, replace=False)).astype(np.int64)
    pos[0], pos[n // 2] = 0, circumference // 2                     # the antipodal pair: D = 32767 occurs
    pos = np.sort(pos)
    a = np.abs(pos[:, None] - pos[None, :])
    return np.minimum(a, circumference - a).astype(np.int16)


def line_metric(n, span=32767, seed=0):
    pos = np.sort(np.random.RandomState(seed).choice(span + 1, size=n, replace=False)).astype(np.int64)
    pos[0], pos[-1] = 0, span
    return np.abs(pos[:, None] - pos[None, :]).astype(np.int16)
