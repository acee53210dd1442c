"""mo3d::OctreeIndex::insertLeaf / levelDepth (include/hpmvs/Scene.h; tests/octree_index_insert.cpp, a g++ program that links no
library) against hpmvs_amd.frontier.Octree.insert: 2 000 random insertions down to depth 21, the key of all ones among them -- the
branch and leaf key sets equal after every hundredth step and at the end, no key entered twice, the vectors only ever appended
to -- and levelDepth against the halving chain Cell(parent, idx) makes."""
import os
import struct
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
ALL_ONES = (1 << 64) - 1          # depth 21, every child bit set


def _insertions(n):
    """n keys frontier.Octree.insert accepts one after the other, and the tree's sets after every hundredth and the last."""
    from hpmvs_amd import frontier
    rng = np.random.default_rng(5)
    O = frontier.Octree(np.zeros(3, f32), f32(3.0))
    keys, snaps = [], {}
    while len(keys) < n:
        if not keys:
            key = ALL_ONES
        else:
            # below the root, or below a branch that is there already: prefixes are shared, most of them exist when a key arrives
            k = keys[int(rng.integers(len(keys)))]
            d0 = int(rng.integers(0, frontier.key_depth(k)))          # a proper prefix of an earlier key: the root or a branch
            base = k >> (3 * (frontier.key_depth(k) - d0))
            key = base
            for _ in range(int(rng.integers(1, 22 - d0)) if d0 < 21 else 0):
                key = (key << 3) | int(rng.integers(8))
        # a branch, a nonempty leaf, or below one: no insertion addConditional could have made
        if key in O.branches or any((key >> (3 * j)) in O.leaves for j in range(frontier.key_depth(key))):
            continue
        O.insert(key, len(keys))
        keys.append(key)
        if len(keys) % 100 == 0 or len(keys) == n:
            snaps[len(keys) - 1] = (set(O.branches), set(O.leaves))
    return keys, snaps


def test_insert_leaf_equals_octree_insert(tmp_path):
    exe = str(tmp_path / "octree_index_insert")
    subprocess.run(["g++", "-std=c++14", "-O2", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "octree_index_insert.cpp"),
                    "-o", exe], check=True, capture_output=True)
    n = 2000
    keys, snaps = _insertions(n)
    from hpmvs_amd import frontier
    depths = [frontier.key_depth(k) for k in keys]
    assert keys[0] == ALL_ONES and max(depths) == 21 and min(depths) <= 2 and len(set(keys)) == n
    W = f32(3.0)
    chain = [W]
    for _ in range(21):
        chain.append(f32(float(chain[-1]) / 2.0))
    widths = chain + [np.nextafter(w, f32(np.inf)) for w in chain[1:]] + [np.nextafter(w, f32(0)) for w in chain[1:]] + \
        [f32(float(w) * 0.9) for w in chain[1:]] + [f32(0), f32(np.nan), f32(np.inf), f32(float(chain[21]) / 2.0)]
    want_depth = [-1] + list(range(1, 22)) + [-1] * (len(widths) - 22)
    inp, outp = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(inp, "wb") as f:
        f.write(struct.pack("fi", float(W), n) + np.array(keys, np.uint64).tobytes())
        f.write(struct.pack("i", len(widths)) + np.array(widths, f32).tobytes())
    r = subprocess.run([exe, str(inp), str(outp)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    buf = open(outp, "rb").read()
    off, seen, prev_b, prev_l = 0, 0, [], []
    while seen < len(snaps):
        step, nb, nl = struct.unpack_from("iii", buf, off)
        off += 12
        b = np.frombuffer(buf, np.uint64, nb, off).tolist(); off += 8 * nb
        l = np.frombuffer(buf, np.uint64, nl, off).tolist(); off += 8 * nl
        want_b, want_l = snaps[step]
        assert len(b) == len(set(b)) and len(l) == len(set(l)), (step, "a key was entered twice")
        assert set(b) == want_b and set(l) == want_l, (step, len(b), len(want_b))
        assert b[:len(prev_b)] == prev_b and l[:len(prev_l)] == prev_l and l == keys[:step + 1], (step, "append only")
        prev_b, prev_l = b, l
        seen += 1
    assert seen == n // 100 and ALL_ONES in prev_l
    got = np.frombuffer(buf, np.int32, len(widths), off).tolist()
    assert off + 4 * len(widths) == len(buf) and got == want_depth, [(float(w), g, d) for w, g, d in zip(widths, got, want_depth) if g != d]
