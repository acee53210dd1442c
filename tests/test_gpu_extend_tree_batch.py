"""api.extend_tree_batch / hpmvs_extend_tree_batch against the composition of the four calls it replaces, written out here:
hpmvs_expand_batch with everything skipped (the centres before optimize) -> hpmvs_octree_locate_batch -> hpmvs_expand_batch with
the tree's skip bytes -> hpmvs_octree_locate_batch on the refined centres.  Scenes, trees and levels are those of
tests/test_gpu_extend_level_tree.py: BASELINE configs[0] and the 12-view scene through seed_tree, the whole tree and the subtree
root that file picks, the two lowest populated levels.  Host pointers and device pointers; every field of `out` and every key
array byte for byte (pre_key where pre_inside, border / post_key where ok -- the call writes 0 elsewhere, which is compared too);
guard bytes behind every output; NULL key pointers one at a time; the refusals leave poisoned outputs untouched.

Non-vacuity is asserted on the composition alone, summed over the cases: a skip by a nonempty leaf, a skip by finer structure, a
centre before optimize outside the root, a refined candidate addConditional refuses, a refined border candidate."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_extend_level_tree import CASES, level_parents, make_seed_batch, subtree_root, two_lowest_levels

pytestmark = pytest.mark.gpu
f32 = np.float32
HPMVS_ERR_ARG = -2
GUARD = 16            # rows behind every output
POISON = 0x5A
KEYS = (("skip", np.uint8), ("pre_inside", np.uint8), ("pre_key", np.uint64), ("border", np.uint8), ("post_key", np.uint64))
FIELDS = (("center", f32, 4), ("normal", f32, 4), ("scale", f32, 1), ("n_images", np.int32, 1), ("images", np.int32, None),
          ("ok", np.uint8, 1), ("color", f32, 3), ("ncc", f32, 1), ("fmin", np.float64, 1), ("x", np.float64, 3),
          ("result", np.int32, 1), ("nevals", np.int32, 1), ("stage", np.int32, 1), ("ngrabs", np.int32, 1))


def composition(g, parents, width, rc, rw, bk, lk):
    """The four calls; -> (out Batch, dict of the five key arrays as the fused call defines them)."""
    from hpmvs_amd import api
    n, N = parents.n, 6 * parents.n
    width = f32(width)
    add_width = f32(float(width) * 0.9)
    cc, cw = np.zeros((n, 3), f32), np.full(n, width, f32)
    pre = api.expand_batch(g, api.EXPAND_EXTEND, parents, cc, cw, np.ones(N, np.uint8))
    a = api.octree_locate_batch(g, rc, rw, bk, lk, pre.center, add_width)
    inside = a.inside != 0
    nonempty, finer = inside & (a.leaf_index >= 0), inside & (a.leaf_width < width)
    skip = (nonempty | finer).astype(np.uint8)                                   # CellProcessor.cpp:124
    out = api.expand_batch(g, api.EXPAND_EXTEND, parents, cc, cw, skip)
    b = api.octree_locate_batch(g, rc, rw, bk, lk, out.center, add_width)
    ok = out.ok != 0
    border = ok & (b.inside == 0)                                                # :147
    keys = dict(skip=skip, pre_inside=a.inside.copy(), pre_key=a.target_key * inside.astype(np.uint64),
                border=border.astype(np.uint8), post_key=b.target_key * (ok & ~border).astype(np.uint64))
    tally = dict(skip_nonempty=int(nonempty.sum()), skip_finer=int(finer.sum()), outside_pre=int((~inside).sum()),
                 refined_refused=int((ok & ~border & (b.target_key == 0)).sum()), refined_border=int(border.sum()))
    return out, keys, tally


@pytest.fixture(scope="module")
def cases():
    """Per scene the GPU scene and its refined seeds; per (scene, whole / subtree, level) the parents, the tree as key arrays, the
    level width and the composition's result, computed once."""
    from hpmvs_amd import api, frontier, synth
    scenes, out = [], []
    for tag, c in CASES.items():
        scene = synth.make_scene(c["views"], 640, 480, n_waves=24)
        g = api.Scene(scene, device=0)
        scenes.append(g)
        b = make_seed_batch(scene, c["groups"])
        api.optimize_batch(g, b)
        k = np.nonzero(b.ok)[0]
        R = api.Batch(b.center[k], b.normal[k], b.scale[k], b.n_images[k], b.images[k])
        R.ok[:] = 1
        T = frontier.seed_tree(g, R, patch_init_maxlevel=c["maxlevel"], set_depths=False)
        O = frontier.Octree.from_seed_tree(T)
        for whole in (True, False):
            root = subtree_root(O, 0 if whole else c["sub_depth"])
            S = O.subtree(root) if root != 1 else O
            bk, lk = S.branch_keys(), S.leaf_table()[0]
            for depth in two_lowest_levels(S):
                keys, leaves = level_parents(S, T, depth)
                parents = frontier._rows(R, [int(T.rows[T.cell_start[l]]) for l in leaves])
                if tag == "configs0" and whole:
                    parents.n_images[0] = 0       # a parent that cannot be expanded: its six candidates keep -20 -> 0 whatever the tree says
                width = S.cell(keys[0])[1]
                want, wkeys, tally = composition(g, parents, width, S.root_center, S.root_width, bk, lk)
                out.append(dict(what=(tag, "whole" if whole else "subtree", depth), g=g, parents=parents, width=f32(width),
                                rc=S.root_center.copy(), rw=f32(S.root_width), bk=bk, lk=lk, want=want, keys=wkeys, tally=tally))
    yield out
    for g in scenes:
        g.close()


def test_the_composition_shows_every_case(cases):
    total = {}
    for c in cases:
        for k, v in c["tally"].items():
            total[k] = total.get(k, 0) + v
    print("extend_tree_batch composition tallies", total, [(c["what"], c["parents"].n) for c in cases])
    assert len(cases) == 8 and min(total.values()) >= 1, total


class Buffers:
    """The fourteen arrays of an out batch and the five key arrays, each with GUARD rows behind it, in host memory or on the
    device.  Host: everything poisoned (a staged call returns every byte of the n rows).  Device: the batch rows zero, as a
    staged call would return what no kernel writes, the key rows and every guard poisoned."""

    def __init__(self, n, M, device, n_struct=None, null=()):
        from hpmvs_amd import api
        self.n, self.device = n, device
        self.host, self.dev = {}, {}
        for name, dt, cols in FIELDS + tuple((k, d, 1) for k, d in KEYS):
            a = np.full((n + GUARD, M if cols is None else cols), POISON, np.uint8).repeat(np.dtype(dt).itemsize, axis=1)
            if device and name not in dict(KEYS):
                a[:n] = 0
            self.host[name] = a
        self.start = {k: v.copy() for k, v in self.host.items()}
        if device:
            import torch
            self.torch = torch
            self.dev = {k: torch.from_numpy(v).to("cuda:0") for k, v in self.host.items()}
        ptr = (lambda k: self.dev[k].data_ptr()) if device else (lambda k: self.host[k].ctypes.data)
        self.pb = api.PatchBatch()
        self.pb.n, self.pb.max_images = (n if n_struct is None else n_struct), M
        for name, _, _ in FIELDS:
            setattr(self.pb, name, ptr(name))
        self.kb = api.ExtendTreeKeysStruct()
        for name, _ in KEYS:
            setattr(self.kb, name, None if name in null else ptr(name))

    def fetch(self):
        if self.device:
            self.torch.cuda.synchronize()
            self.host = {k: v.cpu().numpy() for k, v in self.dev.items()}

    def rows(self, name):
        dt = dict((k, d) for k, d, _ in FIELDS + tuple((k, d, 1) for k, d in KEYS))[name]
        return self.host[name][:self.n].copy().view(dt)

    def touched(self, names=None, whole=False):
        """The arrays (of `names`, default all) whose guard rows -- whole: any row -- differ from what they started as."""
        return [k for k in (self.host if names is None else names) if not np.array_equal(self.host[k][0 if whole else self.n:], self.start[k][0 if whole else self.n:])]


def fused(c, device, null=(), width=None, rc=None, rw=None, bk=None, lk=None, parents=None, n_struct=None):
    """One hpmvs_extend_tree_batch through api.lib() on poisoned, over-allocated outputs -> (status, Buffers)."""
    from hpmvs_amd import api
    parents = c["parents"] if parents is None else parents
    bk = c["bk"] if bk is None else np.ascontiguousarray(bk, np.uint64)
    lk = c["lk"] if lk is None else np.ascontiguousarray(lk, np.uint64)
    B = Buffers(6 * parents.n, parents.max_images, device, n_struct, null)
    keep = []
    if device:
        import torch
        up = lambda a: keep.append(torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to("cuda:0")) or keep[-1].data_ptr()
        pb = api.PatchBatch()
        pb.n, pb.max_images = parents.n, parents.max_images
        for name in api.Batch.FIELDS:
            setattr(pb, name, up(getattr(parents, name)) if getattr(parents, name).size else None)
        dbk, dlk = np.zeros(0, np.uint64), np.zeros(0, np.uint64)
        t = api._octree_index(c["rc"] if rc is None else rc, c["rw"] if rw is None else rw, dbk, dlk)
        t.n_branches, t.n_leaves = len(bk), len(lk)
        t.branch_key, t.leaf_key = (up(bk) if len(bk) else None), (up(lk) if len(lk) else None)
        torch.cuda.synchronize()
        stream = torch.cuda.Stream(device="cuda:0")
        sp = C.c_void_p(stream.cuda_stream)
    else:
        pb = parents.c_struct()
        t = api._octree_index(c["rc"] if rc is None else rc, c["rw"] if rw is None else rw, bk, lk)
        sp = None
    o = api.default_options()
    status = api.lib().hpmvs_extend_tree_batch(c["g"].h, C.byref(o), C.byref(t), C.byref(pb), float(c["width"] if width is None else width),
                                               C.byref(B.pb), C.byref(B.kb), 1 if device else 0, sp)
    if device:
        stream.synchronize()
    B.fetch()
    return status, B


def assert_equals_composition(B, want, wkeys, what, null=()):
    for name, _, _ in FIELDS:
        a, b = B.rows(name), np.ascontiguousarray(getattr(want, name)).reshape(want.n, -1)
        assert a.tobytes() == b.tobytes(), (what, name, np.nonzero((a != b).any(axis=1))[0][:8])
    for name, _ in KEYS:
        if name in null:
            continue
        a, b = B.rows(name).reshape(-1), wkeys[name]
        assert a.tobytes() == b.tobytes(), (what, name, np.nonzero(a != b)[0][:8])
    assert B.touched() == [], (what, "guard rows written", B.touched())
    assert B.touched(null, whole=True) == [], (what, "a NULL output was written")


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_fused_call_equals_the_four_calls(cases, device):
    from hpmvs_amd import api
    for c in cases:
        status, B = fused(c, device)
        assert status == 0, (c["what"], api.lib().hpmvs_last_error())
        assert_equals_composition(B, c["want"], c["keys"], c["what"])


def test_api_extend_tree_batch_equals_the_four_calls(cases):
    from hpmvs_amd import api
    c = cases[0]
    out, k = api.extend_tree_batch(c["g"], c["parents"], c["width"], c["rc"], c["rw"], c["bk"], c["lk"])
    for name in api.Batch.FIELDS:
        assert getattr(out, name).tobytes() == getattr(c["want"], name).tobytes(), name
    for name, _ in KEYS:
        assert getattr(k, name).tobytes() == c["keys"][name].tobytes(), name


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_null_key_pointers_one_at_a_time(cases, device):
    from hpmvs_amd import api
    c = min(cases, key=lambda c: c["parents"].n)
    for name, _ in KEYS:
        status, B = fused(c, device, null=(name,))
        assert status == 0, (name, api.lib().hpmvs_last_error())
        assert_equals_composition(B, c["want"], c["keys"], (c["what"], "without", name), null=(name,))


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_refusals_write_nothing(cases, device):
    c = min(cases, key=lambda c: c["parents"].n)
    lk, bk = c["lk"], c["bk"]
    deepest = int(max(lk))
    bad_root = c["rc"].copy()
    bad_root[1] = np.nan
    refusals = {
        "0.9 width": dict(width=f32(float(c["width"]) * 0.9)),
        "width next to a level width": dict(width=np.nextafter(c["width"], f32(np.inf))),
        "root width as width": dict(width=c["rw"]),
        "NaN width": dict(width=f32(np.nan)),
        "duplicated leaf key": dict(lk=np.concatenate([lk, lk[:1]])),
        "duplicated branch key": dict(bk=np.concatenate([bk, bk[:1]])),
        "orphan key": dict(lk=np.concatenate([lk, [np.uint64((deepest << 6) | 0o11)]]) if deepest < (1 << 57) else None),
        "root centre not finite": dict(rc=bad_root),
        "root width not finite": dict(rw=f32(np.inf)),
        "out->n != 6 n": dict(n_struct=6 * c["parents"].n - 1),
    }
    for what, kw in refusals.items():
        assert all(v is not None for v in kw.values()), what
        status, B = fused(c, device, **kw)
        assert status == HPMVS_ERR_ARG, what
        assert B.touched(whole=True) == [], (what, B.touched(whole=True))


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_no_parents_and_the_empty_tree_succeed(cases, device):
    from hpmvs_amd import api, frontier
    c = min(cases, key=lambda c: c["parents"].n)
    status, B = fused(c, device, parents=frontier._rows(c["parents"], []))
    assert status == 0, api.lib().hpmvs_last_error()
    assert B.touched(whole=True) == []
    none = np.zeros(0, np.uint64)
    want, wkeys, tally = composition(c["g"], c["parents"], c["width"], c["rc"], c["rw"], none, none)
    assert tally["skip_nonempty"] == 0 and tally["skip_finer"] == 0 and tally["refined_refused"] == 0 and want.ok.any()
    status, B = fused(c, device, bk=none, lk=none)
    assert status == 0, api.lib().hpmvs_last_error()
    assert_equals_composition(B, want, wkeys, "the empty tree")
