"""mo3d::OctreeIndex::applySweep (include/hpmvs/Scene.h; tests/octree_index_sweep.cpp, a g++ program that links no library)
against hpmvs_amd.frontier.apply_sweep on frontier.Octree: random sweeps one after the other on one tree -- removals (with the
one-level collapse of an emptied parent), splits with no, one and several children, two children in one leaf -- the branch and
leaf key sets equal after every sweep, the surviving keys in their old order, the new leaves named by the child they came from.
A sweep that names a key that is no nonempty leaf changes nothing."""
import os
import struct
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def _tree(rng, n):
    from hpmvs_amd import frontier
    O = frontier.Octree(np.zeros(3, f32), f32(8.0))
    while len(O.leaves) < n:
        key = 1
        for _ in range(int(rng.integers(2, 6))):
            key = (key << 3) | int(rng.integers(8))
        if key in O.branches or any((key >> (3 * j)) in O.leaves for j in range(frontier.key_depth(key))):
            continue
        O.insert(key, len(O.leaves))
    return O


def _sweep(rng, O, bad=False):
    keys = [k for k in O.leaves if rng.random() < 0.6]
    rng.shuffle(keys)
    n = len(keys)
    removed, split = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    child, child_key = np.zeros((n, 4), np.uint8), np.zeros((n, 4), np.uint64)
    for i, key in enumerate(keys):
        r = rng.random()
        if r < 0.45:
            removed[i] = 1
        elif r < 0.8:
            split[i] = 1
            child[i] = rng.random(4) < 0.5
            octs = rng.integers(0, 8, 4)
            if rng.random() < 0.4:
                octs[1] = octs[0]
            for k in range(4):
                if child[i, k]:
                    child_key[i, k] = (key << 3) | int(octs[k])
    if bad and n:
        keys[n // 2] = (keys[n // 2] << 3) | 1                             # no leaf of the tree
        removed[n // 2], split[n // 2] = 1, 0
    return np.array(keys, np.uint64), removed, split, child, child_key


def test_apply_sweep_equals_octree(tmp_path):
    from hpmvs_amd import frontier
    exe = str(tmp_path / "octree_index_sweep")
    subprocess.run(["g++", "-std=c++14", "-O2", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "octree_index_sweep.cpp"),
                    "-o", exe], check=True, capture_output=True)
    rng = np.random.default_rng(31)
    O = _tree(rng, 600)
    inp, outp = tmp_path / "in.bin", tmp_path / "out.bin"
    bk, lk = sorted(O.branches), list(O.leaves)
    blob = struct.pack("ii", len(bk), len(lk)) + np.array(bk, np.uint64).tobytes() + np.array(lk, np.uint64).tobytes()
    sweeps, want = [], []
    for s in range(6):
        bad = s == 3
        keys, removed, split, child, child_key = _sweep(rng, O, bad)
        sweeps.append(struct.pack("i", len(keys)) + keys.tobytes() + removed.tobytes() + split.tobytes() + child.tobytes() + child_key.tobytes())
        before = list(O.leaves)
        if not bad:
            frontier.apply_sweep([O], np.zeros(len(keys), np.int32), keys, removed, split, child, child_key)
        want.append((not bad, set(O.branches), dict(O.leaves), before, int(removed.sum()), int(split.sum())))
    with open(inp, "wb") as f:
        f.write(blob + struct.pack("i", len(sweeps)) + b"".join(sweeps))
    r = subprocess.run([exe, str(inp), str(outp)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    buf = open(outp, "rb").read()
    off, prev_l, collapsed = 0, lk, 0
    for s, (ok, branches, leaves, before, n_removed, n_split) in enumerate(want):
        got_ok, nb, nl = struct.unpack_from("iii", buf, off); off += 12
        b = np.frombuffer(buf, np.uint64, nb, off).tolist(); off += 8 * nb
        l = np.frombuffer(buf, np.uint64, nl, off).tolist(); off += 8 * nl
        frm = np.frombuffer(buf, np.int32, nl, off).tolist(); off += 4 * nl
        assert bool(got_ok) == ok, s
        assert len(set(b)) == len(b) and len(set(l)) == len(l), s
        assert set(b) == branches and set(l) == set(leaves), (s, len(b), len(branches))
        if not ok:
            assert l == prev_l
            continue
        kept = [k for k, src in zip(l, frm) if src >= 0]
        assert kept == [k for k in prev_l if k in leaves] and [prev_l[src] for src in frm if src >= 0] == kept, s   # the old order
        for k, src in zip(l, frm):
            if src < 0:                                                    # born in this sweep: the row names the first child
                assert leaves[k] == ("branch", -src - 1), (s, k)
        collapsed += sum(1 for k in before if k not in leaves and (k >> 3) != 1 and (k >> 3) not in branches)
        prev_l = l
        assert n_removed > 10 and n_split > 10, s
    assert off == len(buf) and collapsed > 0
