"""A third reading of the two wire formats of the per-round exchange, written from include/hpmvs_amd.h alone:
`hpmvs_record` (192 bytes) and `hpmvs_record_tail` (392 bytes).  Plain numpy, one patch at a time, no torch: it shares
nothing with the kernels of hpmvs_amd/csrc/kernels_basic.hip nor with hpmvs_amd/distributed.py, which are both tested
against it (tests/test_cpu_record_ref.py, tests/test_gpu_record_exchange.py).

The header's rules as applied here:
  * unused id slots are 0xFFFF, pad bytes are zero;
  * a record carries the true n_images as 16 bits and the first min(n_images, 64, max_images) ids;
  * a tail exists only for ok != 0 (or `ok` absent) and 64 < n_images <= min(max_images, 256); tails come in patch
    order; count = n_images - 64;
  * absent color / fmin / ok pack as zeros and are not written on unpack;
  * on unpack a tail whose patch_offset + patch falls outside the batch is dropped, and one whose count exceeds the 192
    ids a tail holds is rejected whole.

The seeded case generators live here too, so that the CPU and the GPU tests see the same inputs.
"""
import functools

import numpy as np

RECORD_IMAGES = 64                       # HPMVS_RECORD_IMAGES
MAX_IMAGES = 256                         # HPMVS_MAX_IMAGES
TAIL_IDS = MAX_IMAGES - RECORD_IMAGES    # ids in one hpmvs_record_tail
NO_IMAGE = 0xFFFF
OPTIONALS = ("color", "fmin", "ok")

# typedef struct hpmvs_record: offsets as the C layout rules give them (fmin is 8-aligned at 48, images at 64)
RECORD = np.dtype(dict(
    names=["center", "normal", "color", "scale", "fmin", "ok", "pad0", "n_images", "pad1", "images"],
    formats=[("<f4", (4,)), ("<f4", (4,)), ("<f4", (3,)), "<f4", "<f8", "u1", "u1", "<u2", ("u1", (4,)), ("<u2", (RECORD_IMAGES,))],
    offsets=[0, 16, 32, 44, 48, 56, 57, 58, 60, 64], itemsize=192))
# typedef struct hpmvs_record_tail
TAIL = np.dtype(dict(names=["patch", "count", "pad", "images"], formats=["<i4", "<u2", "<u2", ("<u2", (TAIL_IDS,))],
                     offsets=[0, 4, 6, 8], itemsize=392))


def pack_records(n, max_images, center, normal, scale, n_images, images, color=None, fmin=None, ok=None):
    """SoA batch of n patches (rows of `images` are max_images wide) -> n hpmvs_record."""
    out = np.zeros(n, RECORD)
    for i in range(n):
        out["center"][i] = center[i]
        out["normal"][i] = normal[i]
        if color is not None:
            out["color"][i] = color[i]
        out["scale"][i] = scale[i]
        if fmin is not None:
            out["fmin"][i] = fmin[i]
        if ok is not None:
            out["ok"][i] = ok[i]
        nim = int(n_images[i])
        out["n_images"][i] = nim & 0xFFFF
        out["images"][i] = NO_IMAGE
        for k in range(max(0, min(nim, RECORD_IMAGES, max_images))):
            out["images"][i, k] = int(images[i, k]) & 0xFFFF
    return out


def has_tail(i, max_images, n_images, ok=None):
    if ok is not None and ok[i] == 0:
        return False
    return RECORD_IMAGES < int(n_images[i]) <= min(max_images, MAX_IMAGES)


def pack_tails(n, max_images, n_images, images, ok=None):
    """The tails of the first n patches, in patch order."""
    rows = [i for i in range(n) if has_tail(i, max_images, n_images, ok)]
    out = np.zeros(len(rows), TAIL)
    for t, i in enumerate(rows):
        count = int(n_images[i]) - RECORD_IMAGES
        out["patch"][t] = i
        out["count"][t] = count
        out["images"][t] = NO_IMAGE
        for k in range(count):
            out["images"][t, k] = int(images[i, RECORD_IMAGES + k]) & 0xFFFF
    return out


def unpack_records(records, batch):
    """records -> rows 0 .. len(records) - 1 of `batch` (a dict of arrays; an optional array that is None is not written)."""
    max_images = batch["images"].shape[1]
    for i in range(len(records)):
        r = records[i]
        batch["center"][i] = r["center"]
        batch["normal"][i] = r["normal"]
        if batch.get("color") is not None:
            batch["color"][i] = r["color"]
        batch["scale"][i] = r["scale"]
        if batch.get("fmin") is not None:
            batch["fmin"][i] = r["fmin"]
        if batch.get("ok") is not None:
            batch["ok"][i] = r["ok"]
        nim = int(r["n_images"])
        batch["n_images"][i] = nim - 65536 if nim >= 32768 else nim   # signed: rejection codes travel as negative counts
        for k in range(max_images):
            slot = int(r["images"][k]) if k < RECORD_IMAGES else NO_IMAGE
            batch["images"][i, k] = -1 if slot == NO_IMAGE else slot
    return batch


def unpack_tails(tails, patch_offset, batch, n=None):
    """ids 64.. of patch (patch_offset + tail.patch) of a batch of n patches (default: every row of batch["images"])."""
    n = batch["images"].shape[0] if n is None else n
    max_images = batch["images"].shape[1]
    for t in range(len(tails)):
        i = patch_offset + int(tails["patch"][t])
        count = int(tails["count"][t])
        if i < 0 or i >= n or count > TAIL_IDS:
            continue
        for k in range(count):
            if RECORD_IMAGES + k < max_images:
                batch["images"][i, RECORD_IMAGES + k] = int(tails["images"][t, k])
    return batch


def sentinel_batch(n, max_images, absent=()):
    """A destination batch that no unpack has touched: -7 in the numeric columns, 0x5A in `ok`, None for absent optionals."""
    b = dict(center=np.full((n, 4), -7, np.float32), normal=np.full((n, 4), -7, np.float32), scale=np.full(n, -7, np.float32),
             n_images=np.full(n, -7, np.int32), images=np.full((n, max_images), -7, np.int32), ok=np.full(n, 0x5A, np.uint8),
             color=np.full((n, 3), -7, np.float32), fmin=np.full(n, -7.0))
    for k in absent:
        b[k] = None
    return b


# ---- cases -------------------------------------------------------------------------------------------------------------
class Case:
    """One generated input.  `arrays` always holds every column (rows >= n are an over-allocation that the product must
    ignore); `absent` names the optional arrays the case hands over as NULL; `shards` are the [lo, hi) cuts of a round;
    `expect` says what the tail list is about: "many" (> 20 tails), "one", "zero", or "any" (cases that are not about the
    list's length)."""

    def __init__(self, name, n, max_images, arrays, absent=(), shards=None, expect="any"):
        self.name, self.n, self.max_images, self.arrays = name, n, max_images, arrays
        self.absent, self.shards, self.expect = tuple(absent), shards, expect

    def col(self, key, lo=0, hi=None):
        """Rows [lo, hi) of one column, or None for an absent optional."""
        if key in self.absent:
            return None
        return self.arrays[key][lo:self.n if hi is None else hi]

    def ref_records(self, lo=0, hi=None):
        hi = self.n if hi is None else hi
        c = lambda k: self.col(k, lo, hi)
        return pack_records(hi - lo, self.max_images, c("center"), c("normal"), c("scale"), c("n_images"), c("images"),
                            color=c("color"), fmin=c("fmin"), ok=c("ok"))

    def ref_tails(self, lo=0, hi=None):
        hi = self.n if hi is None else hi
        return pack_tails(hi - lo, self.max_images, self.col("n_images", lo, hi), self.col("images", lo, hi),
                          ok=self.col("ok", lo, hi))


def _columns(rng, rows, max_images, n_images, ok, garbage):
    """Random columns; ids are drawn from 0..65534.  `garbage` leaves ids in the slots past a row's count (the packers must
    not let them through), otherwise those slots hold -1 as a freshly unpacked batch would."""
    images = rng.integers(0, 65535, (rows, max_images)).astype(np.int32)
    if not garbage:
        images[np.arange(max_images)[None, :] >= np.clip(n_images, 0, None)[:, None]] = -1
    return dict(center=rng.random((rows, 4), dtype=np.float32), normal=rng.random((rows, 4), dtype=np.float32) - 0.5,
                scale=rng.random(rows, dtype=np.float32), n_images=n_images.astype(np.int32), images=images,
                ok=ok.astype(np.uint8), color=rng.random((rows, 3), dtype=np.float32), fmin=rng.random(rows) - 0.25)


SCAN_SIZES = (1, 63, 64, 65, 16383, 16384, 16385, 16448, 32769)   # 256 blocks of 64 exactly, 257, and three chunks of 256 blocks
SCAN_PATTERNS = ("a", "b", "c", "d")
SCAN_MAX_IMAGES = 70


@functools.lru_cache(maxsize=None)
def scan_case(n, pattern):
    """Inputs of hpmvs_pack_record_tails at max_images = 70.  Patterns:
      a  random: ~15 % of the lists long (60 % where n < 1000, so that the list is not trivial); where the batch
         has more than 256 blocks, blocks 250..252 (and 508..510) hold no tail and block 256 (and 511) is all tails
      b  no tail in the first 256 blocks, tails only after them (~30 %, blocks 256, 300 and 512 all tails)
      c  every patch long and ok: n_tails == n
      d  tails only in the last block, its last valid lane among them
      z  no long list at all
    In every pattern the arrays are over-allocated past n by up to two blocks of rows with long, ok lists: a packer that
    looks past b.n finds tails there."""
    m = SCAN_MAX_IMAGES
    rng = np.random.default_rng([n, ord(pattern)])
    nb = (n + 63) // 64
    rows = nb * 64 + 64
    idx = np.arange(rows)
    blk = idx // 64
    short = rng.integers(-2, RECORD_IMAGES + 1, rows)
    long = rng.integers(RECORD_IMAGES + 1, m + 1, rows)
    ok = rng.random(rows) < 0.85
    if pattern == "a":
        is_long = rng.random(rows) < (0.15 if n >= 1000 else 0.6)
        over = rng.random(rows) < 0.02          # n_images > max_images: refused, no tail
        long = np.where(over, rng.integers(m + 1, 400, rows), long)
        full = np.isin(blk, (256, 511))
        empty = np.isin(blk, (250, 251, 252, 508, 509, 510))
        if n == 1:
            full = idx == 0
        is_long = (is_long | full) & ~empty
        ok = ok | full
        long = np.where(full, np.clip(long, None, m), long)
        expect = "one" if n == 1 else "many"
    elif pattern == "b":
        is_long = (blk >= 256) & (rng.random(rows) < 0.3)
        full = np.isin(blk, (256, 300, 512))
        is_long = is_long | full
        ok = ok | full
        expect = "zero" if n <= 16384 else "one" if n == 16385 else "many"
    elif pattern == "c":
        is_long = np.ones(rows, bool)
        ok = np.ones(rows, bool)
        expect = "one" if n == 1 else "many"
    elif pattern == "d":
        last = blk == nb - 1
        is_long = last & ((rng.random(rows) < 0.6) | (idx == n - 1))
        ok = ok | is_long
        expect = "one" if n - (nb - 1) * 64 == 1 else "many"
    elif pattern == "z":
        is_long = np.zeros(rows, bool)
        expect = "zero"
    else:
        raise ValueError(pattern)
    past = idx >= n
    is_long = is_long | past
    long = np.where(past, np.clip(long, None, m), long)
    ok = ok | past
    n_images = np.where(is_long, long, short)
    return Case(f"scan-{pattern}-{n}", n, m, _columns(rng, rows, m, n_images, ok, garbage=True), expect=expect)


# the cases whose tails cross the scan's 256-block chunks AND meet the carry preconditions of tests/test_cpu_record_ref.py
# (pattern c has no empty run of blocks and pattern d no tail before the last block: they ride along in SCAN_SIZES x SCAN_PATTERNS)
SCAN_CARRY = tuple((n, p) for n in (16448, 32769) for p in ("a", "b"))

WIDTHS = (1, 5, 63, 64, 65, 100, 255, 256)


@functools.lru_cache(maxsize=None)
def width_case(max_images, absent=()):
    """Rows of every width the record and the tail treat differently.  The lists hold every count in [-11, max_images],
    counts of exactly 64, 65, 256 and max_images twice (once refined, once not), and rows whose count exceeds the row
    (max_images + 1, max_images + 9, 300: refused for a tail, the record carries the true count and max_images ids).
    n = 130 where these fit; at max_images = 255 and 256 they are 274 and 279 rows, so n = 300 there."""
    m = max_images
    rng = np.random.default_rng([m, len(absent)] + [OPTIONALS.index(a) for a in absent])
    twice = sorted({c for c in (64, 65, 256, m) if c <= m})
    over = [m + 1, m + 9, 300]
    counts = list(range(-11, m + 1)) + twice + twice + over
    forced_ok = [None] * (m + 12) + [1] * len(twice) + [0] * len(twice) + [1] * len(over)
    n = 130 if len(counts) <= 130 else 300
    fill = n - len(counts)
    counts += list(rng.integers(max(0, min(m, 60)), m + 1, fill))
    forced_ok += [None] * fill
    perm = rng.permutation(n)
    n_images = np.array(counts, np.int64)[perm]
    ok = rng.random(n) < 0.7
    for k, p in enumerate(perm):
        if forced_ok[p] is not None:
            ok[k] = bool(forced_ok[p])
    a = _columns(rng, n, m, n_images, ok, garbage=False)
    j = 0
    for i in range(n):                       # the largest id and ids past 32767, in the record and in the tail
        live = min(int(n_images[i]), m)
        if live > 0 and i % 3 == 0:
            a["images"][i, 0] = 65534
        if live > RECORD_IMAGES:
            if n_images[i] <= m and ok[i]:   # (the rows that send a tail when `ok` is present: the three values in turn)
                a["images"][i, RECORD_IMAGES] = (65534, 32768, 32767)[j % 3]
                j += 1
            if live - 1 > RECORD_IMAGES:
                a["images"][i, live - 1] = 32768 + i
    return Case(f"width-{m}" + "".join("-no" + k for k in absent), n, m, a, absent=absent)


ABSENT_COMBOS = (("color",), ("fmin",), ("ok",), OPTIONALS)
ROUND_SHARDS = ((0, 701), (701, 701), (701, 1437), (1437, 1501))


@functools.lru_cache(maxsize=None)
def round_case():
    """A ragged round: n = 1501 at max_images = 96, cut into shards of 701, 0, 736 and 64 patches.  ~20 % of the lists are
    long; the last shard has long lists too but none of them refined, so it is the one non-empty shard without tails."""
    n, m = 1501, 96
    rng = np.random.default_rng(1501)
    n_images = rng.integers(-3, RECORD_IMAGES + 1, n)
    is_long = rng.random(n) < 0.2
    n_images[is_long] = rng.integers(RECORD_IMAGES + 1, m + 1, int(is_long.sum()))
    over = rng.random(n) < 0.01
    n_images[over] = rng.integers(m + 1, 300, int(over.sum()))
    ok = rng.random(n) < 0.8
    ok[ROUND_SHARDS[-1][0]:] &= n_images[ROUND_SHARDS[-1][0]:] <= RECORD_IMAGES
    return Case("round-1501", n, m, _columns(rng, n, m, n_images, ok, garbage=False), shards=ROUND_SHARDS, expect="many")


CAPACITY_KEY = ("scan", 1000, "a")   # the capacity tests' batch
NO_LONG_KEY = ("scan", 300, "z")     # ... and their batch without a long list


def case_keys():
    """Every case, as a key for `case` (cases are built on first use, not when a test module is collected)."""
    keys = [("scan", n, p) for n in SCAN_SIZES for p in SCAN_PATTERNS] + [CAPACITY_KEY, NO_LONG_KEY]
    keys += [("width", m, ()) for m in WIDTHS] + [("width", 100, absent) for absent in ABSENT_COMBOS]
    return keys + [("round",)]


def case(key):
    return dict(scan=scan_case, width=width_case, round=round_case)[key[0]](*key[1:])


def key_id(key):
    return "-".join("+".join(k) if isinstance(k, tuple) else str(k) for k in key if k != ())
