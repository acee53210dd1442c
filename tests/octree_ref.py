"""Test infrastructure: numpy float32 restatements of the reference's DynOctTree (include/hpmvs/doctree.h, src/hpmvs/doctree.cpp) and
of CellProcessor::regularize (src/hpmvs/CellProcessor.cpp:309-367), leaf by leaf and probe by probe, as the reference runs them.
Elements are indices into a caller's array of patch centres."""
import numpy as np

f32 = np.float32


class Cell:
    __slots__ = ("c", "w", "parent", "idx", "children", "data")

    def __init__(self, c, w, parent=None, idx=0):
        self.c, self.w, self.parent, self.idx = c, w, parent, idx
        self.children = None      # None: a leaf
        self.data = []

    @classmethod
    def child(cls, parent, idx):
        # Cell(parent, idx): double arithmetic, float storage
        w = f32(float(parent.w) / 2.0)
        c = np.array([float(parent.c[k]) + (1.0 if (idx >> k) & 1 else -1.0) * float(w) / 2.0 for k in range(3)], dtype=f32)
        return cls(c, w, parent, idx)

    def make_branch(self):
        self.children = [Cell.child(self, i) for i in range(8)]

    def empty(self):
        if self.children is None:
            return not self.data
        return all(ch.empty() for ch in self.children)


class OctTree:
    def __init__(self, center, width, centres):
        self.root = Cell(np.asarray(center, dtype=f32).copy(), f32(width))
        self.root.make_branch()
        self.P = centres          # [N, >= 3] float32 element centres

    def at(self, p, node=None):
        b = self.root if node is None else node
        while True:
            idx = (int(f32(p[2]) > b.c[2]) << 2) | (int(f32(p[1]) > b.c[1]) << 1) | int(f32(p[0]) > b.c[0])
            ch = b.children[idx]
            if ch.children is None:
                return ch
            b = ch

    def split(self, leaf):
        """Leaf::split: the leaf becomes a Branch with eight empty leaves; its elements are returned."""
        d, leaf.data = leaf.data, []
        leaf.make_branch()
        return d

    def add(self, e, width):
        """DynOctTree::add(e, width)."""
        p = self.P[e]
        leaf = self.at(p)
        while float(leaf.w) / 2.0 > float(width):
            buf = self.split(leaf)
            for x in buf:
                self.at(self.P[x], leaf).data.append(x)
            leaf = self.at(p, leaf)
        leaf.data.append(e)
        return leaf

    def remove(self, leaf):
        """DynOctTree::remove(leaf): clear it; an emptied parent Branch collapses into one empty leaf."""
        leaf.data = []
        par = leaf.parent
        if par is not self.root and par.empty():
            par.children = None
            par.data = []
            return par
        return leaf

    def leaves(self, node=None):
        node = self.root if node is None else node
        if node.children is None:
            yield node
            return
        for ch in node.children:
            yield from self.leaves(ch)

    def nonempty(self, node=None):
        return [l for l in self.leaves(node) if l.data]

    def depth(self, leaf):
        d = 0
        while leaf is not self.root:
            leaf = leaf.parent; d += 1
        return d


def _dot(a, b):
    return (f32(a[0] * b[0]) + f32(a[1] * b[1])) + f32(a[2] * b[2])


def _cross(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], dtype=f32)


def _normalized(a):
    n2 = _dot(a, a)
    if n2 > 0:
        n = np.sqrt(f32(n2))
        return np.array([a[0] / n, a[1] / n, a[2] / n], dtype=f32)
    return a.copy()


def probes(center, normal, cam_xaxis, width):
    """The 24 probe points of regularize, yy outer, xx inner."""
    n = np.asarray(normal[:3], dtype=f32)
    y = _normalized(_cross(n, np.asarray(cam_xaxis[:3], dtype=f32)))
    x = _cross(y, n)
    c = np.asarray(center[:3], dtype=f32)
    w = f32(width)
    out = []
    for yy in range(-2, 3):
        for xx in range(-2, 3):
            if xx == 0 and yy == 0:
                continue
            out.append(np.array([c[k] + (f32(xx) * x[k] + f32(yy) * y[k]) * w for k in range(3)], dtype=f32))
    return out


def regularize(tree, center, normal, cam_xaxis, width, expanded, flatness, order=None):
    """CellProcessor::regularize on `tree`: (flatness, neighbour leaves in first-probe order).  order: None sums in first-probe
    order (the kernel's); a permutation of range(k) sums in that order instead (the reference's std::set order is one)."""
    if not expanded:
        return f32(flatness), None
    found = []
    for p in probes(center, normal, cam_xaxis, width):
        leaf = tree.at(p)
        if leaf.data and not any(leaf is f for f in found):
            found.append(leaf)
    k = len(found)
    if k < 1:
        return f32(2.6), found
    if k < 4:
        return f32(2.5), found
    nn = _normalized(np.asarray(normal[:3], dtype=f32))
    x0 = np.asarray(center[:3], dtype=f32)
    dist = f32(0)
    for j in (range(k) if order is None else order):
        pb = tree.P[found[j].data[0]]
        e = _dot(nn, np.array([pb[0] - x0[0], pb[1] - x0[1], pb[2] - x0[2]], dtype=f32))
        dist = f32(dist + f32(e * e))
    return f32(np.sqrt(f32(dist / f32(k))) / f32(width)), found
