"""Isomap of a point cloud on the GPU.

Tenenbaum, de Silva and Langford's Isomap (the method IsoMap_LE's README names first) and de Silva and Tenenbaum's
landmark form: the k-NN graph of the points (gwamd.pointgraph, gw_nng_*), geodesic distances over it from every
point or from L landmarks (gwamd.geodesics, gw_geo_*: the hot path, in HIP), then landmark MDS in fp64.  device=-1
runs the same steps on the host.

    python -m gwamd.isomap --points X.npy --knn 10 --dimensions 2 [--landmarks L] [--seed 0] [--no-self]
        --output x.emb [--groups g.csv] [--neighbors x.nn] [--device N]
"""
import argparse
import sys

import numpy as np

from .geodesics import Geodesics

try:
    import torch
except Exception:  # pragma: no cover - torch is optional for the host path
    torch = None

# Device (or host) memory the geodesic rows of one chunk of landmarks may take.  A landmark set whose [L][n] float64
# matrix fits is queried once; a larger one is queried in chunks of this size, twice (once for the landmarks' own
# distances, once to place the points), so memory stays under the budget at the price of the second query.
CHUNK_BYTES = 8 << 30


class _Vectors:
    """The part of a solver handle classify.scoring and neighbors.most_similar read: the float32 vectors where they
    lie."""

    def __init__(self, device, y):
        self.device, self.n, self._h = device, y.shape[0], True
        self._v32 = np.ascontiguousarray(y, np.float32)
        self._t = torch.as_tensor(self._v32, device=f"cuda:{device}") if device >= 0 else None

    def vectors_numpy(self):
        return self._v32

    def vectors_torch(self):
        if self._t is None:
            raise ValueError("host evaluation keeps its vectors in host memory (use vectors_numpy())")
        return self._t


class IsomapEmbedding:
    """What isomap() returns: vectors float64 [n][dim] (rows outside the main component all zero), eigenvalues
    float64 [dim] of the landmarks' doubly centred matrix (descending), landmarks and outside (row ids, ascending),
    labels, geodesic stats; classify.scoring and neighbors.most_similar take it as it is."""

    def __init__(self, device, labels, vectors, eigenvalues, landmarks, outside, stats):
        self.labels = labels
        self.vectors = vectors
        self.eigenvalues = eigenvalues
        self.landmarks = landmarks
        self.outside = outside
        self.stats = stats
        self.model = _Vectors(device, vectors)

    def save(self, path):
        """`<rows> <dim>` then `<label> v ... v` (deepsim.save_embeddings' text; classify.read_embedding reads it)."""
        from . import deepsim
        deepsim.save_embeddings(path, self.vectors)


def _fix_signs(y):
    """Per column: the entry of largest magnitude is positive, the lowest row winning ties (as gw_le)."""
    for c in range(y.shape[1]):
        if y[int(np.argmax(np.abs(y[:, c]))), c] < 0:
            y[:, c] = -y[:, c]
    return y


def landmark_mds(query, landmarks, n, dim, device, chunk_bytes=CHUNK_BYTES):
    """Landmark MDS in fp64.  query(rows) gives the distances [len(rows)][n] from landmark rows (a torch CUDA tensor
    for device >= 0, numpy otherwise).  D2 = D[:, landmarks]**2, mu = D2.mean(1), B = -(D2 - row means - column
    means + grand mean) / 2; the top `dim` eigenpairs (lam, V) of B; every point x, the landmarks included, lies at
    lam**-0.5 * V' (mu - D[:, x]**2) / 2.  Returns (y float64 [n][dim] numpy, signs not yet fixed; lam [dim])."""
    L = len(landmarks)
    rows = max(1, int(chunk_bytes) // (8 * n))
    chunks = [landmarks[a:a + rows] for a in range(0, L, rows)]
    on_gpu = device >= 0
    lm = torch.as_tensor(landmarks.astype(np.int64), device=f"cuda:{device}") if on_gpu else landmarks
    kept = None
    if len(chunks) == 1:
        kept = query(chunks[0])
        d2 = kept[:, lm] ** 2
    else:
        cat = torch.cat if on_gpu else np.concatenate
        d2 = cat([query(c)[:, lm] ** 2 for c in chunks])
    mu = d2.mean(1)
    b = -0.5 * (d2 - mu[:, None] - d2.mean(0)[None, :] + d2.mean())
    b = 0.5 * (b + b.T)  # a path added from its other end differs in the last bits: eigh gets the mean of the two
    lam, vec = torch.linalg.eigh(b) if on_gpu else np.linalg.eigh(b)
    lam, vec = (lam.flip(0)[:dim], vec.flip(1)[:, :dim]) if on_gpu else (lam[::-1][:dim], vec[:, ::-1][:, :dim])
    lam_host = lam.cpu().numpy() if on_gpu else np.array(lam)
    if not np.all(lam_host > 0):
        raise ValueError(f"the top {dim} eigenvalues {lam_host} are not all positive: fewer dimensions or more landmarks")
    coef = 0.5 * (vec / lam ** 0.5).T  # [dim][L]
    if kept is not None:
        y = coef @ (mu[:, None] - kept ** 2)
    else:
        y, a = 0.0, 0
        for c in chunks:
            y = y + coef[:, a:a + len(c)] @ (mu[a:a + len(c), None] - query(c) ** 2)
            a += len(c)
    y = y.T
    return np.ascontiguousarray(y.cpu().numpy() if on_gpu else y), lam_host


def isomap(x, k=10, dim=2, landmarks=None, seed=0, device=0, include_self=True, labels=None,
           chunk_bytes=CHUNK_BYTES):
    """Isomap of the points `x` (what eigenmaps.eigenmaps_of_points takes): the union-symmetrised k-NN graph (k
    counts the point itself when include_self), geodesics, landmark MDS.  landmarks: None = every row of the main
    component (classical Isomap); an int L = the first L of np.random.RandomState(seed).permutation(component
    rows), sorted; an array = those rows, which must lie in the main component.  Returns an IsomapEmbedding."""
    from . import pointgraph
    from .neighbors import _vectors_of
    x, device = _vectors_of(x, device)
    n = x.shape[0]
    ids, _, d2 = pointgraph.knn_graph(x, k, 0.0, include_self=include_self, device=device, d2=True)
    g = Geodesics(n, device=device, squared=True, symmetrize="union")
    try:
        g.set_rows(ids, d2)
        comp, main = g.components()
        inside = np.flatnonzero(comp == main).astype(np.int32)
        outside = np.flatnonzero(comp != main).astype(np.int32)
        if landmarks is None:
            lm = inside
        elif np.ndim(landmarks) == 0:
            if not 1 <= int(landmarks) <= len(inside):
                raise ValueError(f"landmarks {landmarks} outside [1, {len(inside)}] (the main component's rows)")
            lm = np.sort(np.random.RandomState(seed).permutation(inside)[:int(landmarks)]).astype(np.int32)
        else:
            lm = np.ascontiguousarray(landmarks, np.int32).reshape(-1)
            if len(lm) == 0 or lm.min() < 0 or lm.max() >= n or np.any(comp[lm] != main):
                raise ValueError("every landmark must be a row of the main component")
        if len(lm) <= dim:
            raise ValueError(f"{len(lm)} landmarks give fewer than {dim} dimensions")
        rounds = relax = falls = 0

        def query(rows):
            nonlocal rounds, relax, falls
            d = g.query(rows, as_torch=device >= 0)
            st = g.stats()
            rounds, relax, falls = max(rounds, st.rounds_max), relax + st.relaxations, falls + st.fallbacks
            return d

        with np.errstate(invalid="ignore", over="ignore"):
            y, lam = landmark_mds(query, lm, n, dim, device, chunk_bytes)
        y[outside] = 0.0
        st = g.stats()
        stats = {"entries": st.entries, "components": st.components, "main_component_size": st.main_component_size,
                 "rounds_max": rounds, "relaxations": relax, "fallbacks": falls}
    finally:
        g.free()
    return IsomapEmbedding(device, [str(i) for i in range(n)] if labels is None else list(labels), _fix_signs(y), lam,
                           lm, outside, stats)


def cli(argv=None):
    ap = argparse.ArgumentParser(description="Isomap of a point cloud on MI355X.")
    ap.add_argument("--points", required=True, help="a .npy matrix [n][d]")
    ap.add_argument("--knn", type=int, default=10, help="neighbours per point, itself included unless --no-self")
    ap.add_argument("--dimensions", type=int, default=2)
    ap.add_argument("--landmarks", type=int, default=None, help="landmark Isomap with this many random landmarks")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--no-self", action="store_true", help="a point is not its own neighbour")
    ap.add_argument("--output", required=True, help="embeddings (classify.read_embedding reads them)")
    ap.add_argument("--groups", default=None, help="lines `node,label`: print classify.scoring's table")
    ap.add_argument("--neighbors", default=None, help="write the top-20 cosine neighbours there")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args(argv)
    pts = np.load(args.points, allow_pickle=False)
    if pts.ndim != 2:
        ap.error("--points must hold a matrix [n][d]")
    emb = isomap(pts, k=args.knn, dim=args.dimensions, landmarks=args.landmarks, seed=args.seed, device=args.device,
                 include_self=not args.no_self)
    emb.save(args.output)
    st = emb.stats
    print(f"{len(emb.vectors)} x {args.dimensions} isomap -> {args.output}: {len(emb.landmarks)} landmarks, "
          f"{st['components']} components, {len(emb.outside)} rows outside the main one, eigenvalues "
          f"{' '.join(f'{v:.6g}' for v in emb.eigenvalues)}, {st['relaxations']} relaxations, {st['rounds_max']} rounds, "
          f"{st['fallbacks']} fallbacks", file=sys.stderr)
    if args.groups:
        from . import classify
        classify.scoring(emb, classify.read_groups(args.groups), device=args.device)
    if args.neighbors:
        from . import neighbors
        neighbors.neighbors_of(emb, args.neighbors, emb.labels, device=args.device)
    return 0


if __name__ == "__main__":
    sys.exit(cli())
