"""A host model of a working set of Context slots, the table of every public entry that writes a slot or builds cached state
on one, hand-written scenarios and seeded random sequences of those entries, and the checker that runs a sequence on a
long-lived context and tests it after every step (tests/test_slot_model_host.py on the CPU with the numpy FakeContext below,
tests/test_gpu_slot_state.py on the GPU).  DESIGN.md, "What a writing entry leaves on its destination slot", is the prose form
of the table; KEEPS below is the executable one and tests/test_slot_model_host.py holds the two together.

THE MODEL does not predict what a filter or an align computes: after a step it downloads the slots the call wrote and takes
what the device returned as the new truth.  What it does predict is the bookkeeping: which slots a call may touch at all, the
size-independent rules for normals (`normals_after`) and the segment table of a shard (`segs_after`), and the preconditions
under which the library accepts the call (`legal`).

THE CHECKS after every step (Checker.step):
  1. clean room: a fresh context gets the step's input slots from the model's host copies -- points, normals, and the segment
     table through set_global_base / append_range -- and runs the same call; return values and every written slot are equal
     bit for bit.  Sums are added in the order of the source set's ordering, which a slot may have inherited from the cloud it
     was posed from: the clean room rebuilds the ordering as the slot got it (Slot.recipe: the coordinates it was built from,
     then the rigid motions since) and only then uploads nothing else -- same points, same ordering, no other history.
  2. untouched slots: every slot of the working set that the call did not write still holds the model's bits.
  3. searches on the long-lived context, over the slots the step touched and one it did not, against the independent
     references: nn both ways and correspondences (both reciprocal settings) against the oracle, knn at k = 1 and 17 against
     normals_ref.knn_brute, radius_outlier_removal with return_index into the filter destination against outlier_ref.radius.
  4. the exported keys of nn_forward_keys carry the model's global numbering: a shard's table, a plain slot's own indices.

A sequence is a plain list of (op, dict of plain arguments); `fmt` prints one so that it can be pasted back as a scenario."""
import hashlib
import math
import struct
import ctypes

import numpy as np

import normals_ref as N
import outlier_ref as O
import reject_cases as RC

F32, F64 = np.float32, np.float64
NONE = N.NONE

CLOUD_SLOTS = tuple(range(8))
QUERY_SLOTS = (8, 9)
FILTER_DST = 10
WORKING = CLOUD_SLOTS + QUERY_SLOTS + (FILTER_DST,)
STAGE = 11                          # the clean room stages the segments of a shard through it; never part of a sequence
SIZES = (3, 65, 257, 700, 1025, 3000)
MAX_POINTS = 8000                   # no slot grows beyond this
MAX_SEGS = 64                       # kMaxSegs
CORR_DIST = 6.0                     # of the correspondences the checker asks for
KNN_KS = (1, 17)
VOLATILE = ("ms", "evals", "timing_ms")      # wall times, and the number of distance evaluations (smaller where a seed helped)
# entries whose return values would be compared by the bar of their own GPU tests instead of bits: none.  The f64
# sums of the moment rows, of GICP's objective and of an iteration's residual are added in the order of the source set's Hilbert
# ordering, and that ordering is built from the coordinates the set had when it was first searched: a posed copy inherits its raw
# scan's.  The clean room therefore rebuilds a slot's ordering the way the slot got it (Slot.recipe) before it compares bits.
NOT_BIT_REPRODUCIBLE = ()


def spacing(n):
    """mean point spacing (mm) of an n-point synthetic view: 1.27 mm at 20 000 points (tests/boundary_cases.py)"""
    return round(1.27 * math.sqrt(20000.0 / max(int(n), 1)), 3)


# ------------------------------------------------------------------ clouds and poses (by name: sequences stay plain)

class Env:
    """what the ops need besides a context: the package (host helpers), the named clouds and poses, the oracle"""

    def __init__(self, mvr, orc=None):
        self.mvr, self.orc = mvr, orc
        self.sp = mvr.synth_params(12, 1)
        self.pivot, self.axis = mvr.synth_prior(self.sp)
        self._clouds, self._refs = {}, {}

    def cloud(self, name):
        """'v<view>:<n>' a synthetic view under the mis-calibrated prior (reject_cases._synth_pair's clouds), 'r<view>:<n>' the
        same view as scanned (posed by the pose 'prior<view>'), 'q:<n>' the checker's queries, 'dirty:<n>' a random cloud with a
        few non-finite points, 'empty'.  -> (points, normals or None)"""
        if name not in self._clouds:
            kind, _, n = name.partition(":")
            n = int(n or 0)
            if name == "empty":
                c = (np.zeros((0, 4), F32), None)
            elif kind == "q":
                # the checker's queries: other samples of the same surfaces (another seed), a third each of views 0, 1 and 2 --
                # no query coincides with a point of the clouds under test, and their neighbours lie in every view
                sp = self.mvr.synth_params(12, 1)
                sp.seed = self.sp.seed + 1000 + n
                parts = [self.mvr.synth_view(sp, v, n - 2 * (n // 3) if v == 0 else n // 3) for v in (0, 1, 2)]
                c = (np.ascontiguousarray(np.concatenate([parts[0]] + [RC._pose(self.mvr, sp, v, parts[v]) for v in (1, 2)]), F32), None)
            elif kind == "dirty":
                rng = np.random.default_rng(9000 + n)
                p = np.ones((n, 4), F32)
                p[:, :3] = (rng.standard_normal((n, 3)) * 30.0 + (0.0, 0.0, 900.0)).astype(F32)
                bad = rng.choice(n, max(1, n // 40), replace=False)
                p[bad, rng.integers(0, 3, len(bad))] = np.array([np.nan, np.inf, -np.inf], F32)[rng.integers(0, 3, len(bad))]
                c = (p, None)
            else:
                view = int(kind[1:])
                p, nr = self.mvr.synth_view(self.sp, view, n, normals=True)
                if kind[0] == "v" and view:
                    p, nr = RC._pose(self.mvr, self.sp, view, p, nr)
                c = (np.ascontiguousarray(p, F32), np.ascontiguousarray(nr, F32))
            self._clouds[name] = c
        return self._clouds[name]

    def pose(self, name):
        """'eye', 'nudge' (a small rigid motion), 'back' (its inverse), 'turn' (0.02 rad about the prior's axis), 'prior<view>'"""
        if name == "eye":
            return np.eye(4)
        if name in ("nudge", "back"):
            a = 3e-3
            T = np.eye(4)
            T[:2, :2] = [[math.cos(a), -math.sin(a)], [math.sin(a), math.cos(a)]]
            T[:3, 3] = (0.25, -0.5, 0.125)
            return T if name == "nudge" else np.linalg.inv(T)
        if name == "turn":
            return self.mvr.axis_rotation(self.pivot, self.axis, 0.02)
        if name.startswith("prior"):
            return self.mvr.axis_rotation(self.pivot, self.axis, self.mvr.turntable_angle(int(name[5:]), 12))
        raise KeyError(name)

    def ref(self, tag, arrays, make):
        """a reference result, computed once per content"""
        h = hashlib.blake2b(digest_size=16)
        h.update(repr(tag).encode())
        for a in arrays:
            h.update(np.ascontiguousarray(a).tobytes())
            h.update(b"|")
        k = h.digest()
        if k not in self._refs:
            self._refs[k] = make()
        return self._refs[k]


def model_normals(pts):
    """the normals upload_normals gives a slot: unit vectors from a fixed centre through its points (a function of the contents)"""
    v = pts[:, :3].astype(F64) - (0.0, 0.0, 900.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        v = v / np.linalg.norm(v, axis=1, keepdims=True)
    out = np.zeros((len(pts), 4), F32)
    out[:, :3] = np.where(np.isfinite(v), v, 0.0).astype(F32)
    return out


# ------------------------------------------------------------------ the model

class Slot:
    def __init__(self, pts=None, nrm=None, segs=(), dirty=False):
        self.pts = np.zeros((0, 4), F32) if pts is None else pts
        self.nrm = nrm                       # None, or one row per point
        self.segs = list(segs)               # [(local_begin, count, global_begin)]: the numbering of a shard; [] = plain
        self.dirty = dirty                   # may hold non-finite points
        # how the slot's ORDERING came about, where it has one (Checker.track): None = none yet, or built from the points as they
        # are; dict(kind="base", pts, chain) = built from pts, the slot then moved by chain = [(method, matrix)]; dict(kind="append",
        # a, b, chain) = a's ordering extended by b's; dict(kind="via", pts, fn, T) = never searched itself, ordered when a posed copy
        # of it was made by fn with T; "unknown" = not reproducible through the public entries (seq_run's model)
        self.recipe = None

    @property
    def n(self):
        return len(self.pts)

    def copy(self):
        c = Slot(self.pts, self.nrm, list(self.segs), self.dirty)
        c.recipe = self.recipe
        return c


class Model:
    def __init__(self):
        self.slots = {s: Slot() for s in WORKING}

    def __getitem__(self, s):
        return self.slots[s]

    def snapshot(self):
        m = Model()
        m.slots = {s: v.copy() for s, v in self.slots.items()}
        return m

    def global_index(self, s, local):
        """the global number of local point indices of slot s under its segment table (the identity without one)"""
        out = np.asarray(local, np.int64).copy()
        done = np.zeros(len(out), bool)
        for lb, cnt, gb in self[s].segs:
            hit = ~done & (out >= lb) & (out - lb < cnt)
            out[hit] = gb + (out[hit] - lb)
            done |= hit
        return out


# ------------------------------------------------------------------ the op table

class Op:
    """one public entry.  kind: 'mutator' (writes a slot) or 'builder' (builds cached state, writes none).
    reads(a) / writes(a): slots of the working set; legal(m, a): None or the reason the call would be refused or is outside
    what the model covers; run(ctx, a, m, env): the call itself, -> its return values; draw(m, rng): arguments for a random
    sequence, or None; src_role: the argument that names a source distinct from the destination (None: there is none);
    dst_role: the argument that names the destination (None: the entry has no output slot)."""

    def __init__(self, name, kind, reads, writes, legal, run, draw, dst_role=None, src_role=None):
        self.name, self.kind, self.reads, self.writes, self.legal, self.run, self.draw = name, kind, reads, writes, legal, run, draw
        self.dst_role, self.src_role = dst_role, src_role


OPS = {}


def _op(name, kind, **kw):
    def deco(run):
        OPS[name] = Op(name, kind, run=run, **kw)
        return run
    return deco


def _first(*reasons):
    for r in reasons:
        if r:
            return r
    return None


def _slot_ok(s, allow=WORKING):
    return None if s in allow else "slot %r outside the working set" % (s,)


def _plain(m, s, what="slot"):
    return "%s %d is a shard" % (what, s) if m[s].segs else None


def _clean(m, *slots):
    for s in slots:
        if m[s].dirty:
            return "slot %d may hold non-finite points" % s
    return None


def _atleast(m, s, k):
    return None if m[s].n >= k else "slot %d holds fewer than %d points" % (s, k)


def _has_normals(m, *slots):
    for s in slots:
        if m[s].nrm is None:
            return "slot %d has no normals" % s
    return None


def _pick(rng, seq):
    seq = list(seq)
    return seq[int(rng.integers(0, len(seq)))] if seq else None


def _nonempty(m, k=1, slots=CLOUD_SLOTS, clean=False, normals=False, plain=False):
    return [s for s in slots if m[s].n >= k and not (clean and m[s].dirty) and not (normals and m[s].nrm is None)
            and not (plain and m[s].segs)]


# ---- mutators: data movement

UPLOAD_CLOUDS = tuple("v%d:%d" % (v, n) for v in (0, 1, 2) for n in SIZES) + ("empty", "dirty:700")


@_op("upload", "mutator", dst_role="slot", reads=lambda a: (), writes=lambda a: (a["slot"],),
     legal=lambda m, a: _slot_ok(a["slot"]),
     draw=lambda m, rng: dict(slot=_pick(rng, CLOUD_SLOTS), cloud=_pick(rng, UPLOAD_CLOUDS)))
def _upload(ctx, a, m, env):
    ctx.upload(a["slot"], env.cloud(a["cloud"])[0])


@_op("clear", "mutator", dst_role="slot", reads=lambda a: (), writes=lambda a: (a["slot"],),
     legal=lambda m, a: _slot_ok(a["slot"]), draw=lambda m, rng: dict(slot=_pick(rng, CLOUD_SLOTS)))
def _clear(ctx, a, m, env):
    ctx.clear(a["slot"])


@_op("reserve", "mutator", dst_role="slot", reads=lambda a: (a["slot"],), writes=lambda a: (a["slot"],),
     legal=lambda m, a: _first(_slot_ok(a["slot"]), None if 0 <= a["cap"] <= 2 * MAX_POINTS else "capacity out of range"),
     draw=lambda m, rng: dict(slot=_pick(rng, CLOUD_SLOTS), cap=int(_pick(rng, (0, 100, 2000, MAX_POINTS + 1000)))))
def _reserve(ctx, a, m, env):
    ctx.reserve(a["slot"], a["cap"])


@_op("copy", "mutator", dst_role="dst", src_role="src", reads=lambda a: (a["src"],), writes=lambda a: (a["dst"],),
     legal=lambda m, a: _first(_slot_ok(a["dst"]), _slot_ok(a["src"]), "dst == src is a no-op" if a["dst"] == a["src"] else None),
     draw=lambda m, rng: (lambda d: dict(dst=d, src=_pick(rng, [s for s in CLOUD_SLOTS if s != d])))(_pick(rng, CLOUD_SLOTS)))
def _copy(ctx, a, m, env):
    ctx.copy(a["dst"], a["src"])


def _append_legal(m, a):
    d, s = a["dst"], a["src"]
    return _first(_slot_ok(d), _slot_ok(s), None if m[d].n + m[s].n <= MAX_POINTS else "would grow beyond MAX_POINTS",
                  "segment table full" if len(m[d].segs) >= MAX_SEGS else None)


@_op("append", "mutator", dst_role="dst", src_role="src", reads=lambda a: (a["dst"], a["src"]), writes=lambda a: (a["dst"],), legal=_append_legal,
     draw=lambda m, rng: dict(dst=_pick(rng, CLOUD_SLOTS), src=_pick(rng, CLOUD_SLOTS)))
def _append(ctx, a, m, env):
    ctx.append(a["dst"], a["src"])


@_op("set_global_base", "mutator", dst_role="slot", reads=lambda a: (a["slot"],), writes=lambda a: (a["slot"],),
     legal=lambda m, a: _first(_slot_ok(a["slot"]), _atleast(m, a["slot"], 1)),
     draw=lambda m, rng: (lambda s: s is not None and dict(slot=s, base=int(_pick(rng, (0, 5000, 123456)))) or None)(_pick(rng, _nonempty(m))))
def _set_global_base(ctx, a, m, env):
    ctx.set_global_base(a["slot"], a["base"])


def _append_range_legal(m, a):
    d, s = a["dst"], a["src"]
    return _first(_slot_ok(d), _slot_ok(s), "append_range refuses dst == src" if d == s else None,
                  None if a["begin"] + a["count"] <= m[s].n else "range outside the source",
                  None if m[d].n + a["count"] <= MAX_POINTS else "would grow beyond MAX_POINTS",
                  "segment table full" if len(m[d].segs) + (1 if not m[d].segs and m[d].n else 0) >= MAX_SEGS else None)


def _append_range_draw(m, rng):
    s = _pick(rng, _nonempty(m, 3))
    if s is None:
        return None
    d = _pick(rng, [x for x in CLOUD_SLOTS if x != s])
    b = int(rng.integers(0, m[s].n - 1))
    return dict(dst=d, src=s, begin=b, count=int(rng.integers(1, m[s].n - b + 1)), base=int(_pick(rng, (0, 777, 40000))))


@_op("append_range", "mutator", dst_role="dst", src_role="src", reads=lambda a: (a["dst"], a["src"]), writes=lambda a: (a["dst"],), legal=_append_range_legal,
     draw=_append_range_draw)
def _append_range(ctx, a, m, env):
    ctx.append_range(a["dst"], a["src"], a["begin"], a["count"], a["base"])


POSES = ("nudge", "back", "turn")


def _xf_draw(m, rng):
    s = _pick(rng, _nonempty(m, 1, clean=True))
    if s is None:
        return None
    return dict(dst=_pick(rng, (s,) + CLOUD_SLOTS), src=s, pose=_pick(rng, POSES))


def _xf_legal(m, a):
    return _first(_slot_ok(a["dst"]), _slot_ok(a["src"]), _clean(m, a["src"]))


@_op("transform", "mutator", dst_role="dst", src_role="src", reads=lambda a: (a["src"],), writes=lambda a: (a["dst"],), legal=_xf_legal, draw=_xf_draw)
def _transform(ctx, a, m, env):
    ctx.transform(a["dst"], a["src"], env.pose(a["pose"]))


@_op("transform_f32", "mutator", dst_role="dst", src_role="src", reads=lambda a: (a["src"],), writes=lambda a: (a["dst"],), legal=_xf_legal, draw=_xf_draw)
def _transform_f32(ctx, a, m, env):
    ctx.transform_f32(a["dst"], a["src"], env.pose(a["pose"]))


def _batch_legal(m, a):
    d, s = a["dst"], a["src"]
    if not (len(d) == len(s) == len(a["pose"])) or not d:
        return "one pose per entry"
    for j in range(len(d)):
        r = _first(_slot_ok(d[j]), _slot_ok(s[j]), _clean(m, s[j]))
        if r:
            return r
        for k in range(len(d)):
            if j != k and (d[j] == d[k] or d[j] == s[k]):
                return "a destination appears twice or is another entry's source"
    return None


def _batch_draw(m, rng):
    src = _nonempty(m, 1, clean=True)
    if not src:
        return None
    a = dict(dst=[], src=[], pose=[])
    free = [s for s in CLOUD_SLOTS]
    rng.shuffle(free)
    for s in src[:3]:
        inplace = bool(rng.integers(0, 2))
        d = s if inplace else next((x for x in free if x not in src[:3] and x not in a["dst"]), None)
        if d is None:
            continue
        a["dst"].append(int(d)); a["src"].append(int(s)); a["pose"].append(_pick(rng, POSES))
    return a if a["dst"] else None


@_op("transform_batch", "mutator", dst_role="dst", src_role="src", reads=lambda a: tuple(a["src"]), writes=lambda a: tuple(a["dst"]), legal=_batch_legal,
     draw=_batch_draw)
def _transform_batch(ctx, a, m, env):
    ctx.transform_batch(a["dst"], a["src"], [env.pose(p) for p in a["pose"]])


# ---- mutators: normals

@_op("upload_normals", "mutator", dst_role="slot", reads=lambda a: (a["slot"],), writes=lambda a: (a["slot"],),
     legal=lambda m, a: _first(_slot_ok(a["slot"]), _atleast(m, a["slot"], 1)),
     draw=lambda m, rng: (lambda s: s is not None and dict(slot=s) or None)(_pick(rng, _nonempty(m))))
def _upload_normals(ctx, a, m, env):
    ctx.upload_normals(a["slot"], model_normals(m[a["slot"]].pts))


@_op("estimate_normals", "mutator", dst_role="slots", reads=lambda a: tuple(a["slots"]), writes=lambda a: tuple(a["slots"]),
     legal=lambda m, a: _first(*[_first(_slot_ok(s), _atleast(m, s, 3), _clean(m, s)) for s in a["slots"]],
                               None if len(set(a["slots"])) == len(a["slots"]) and a["slots"] else "distinct slots expected"),
     draw=lambda m, rng: (lambda ss: ss and dict(slots=[int(s) for s in ss[:int(rng.integers(1, 3))]], k=int(_pick(rng, (8, 20)))) or None)(
         list(rng.permutation(_nonempty(m, 3, clean=True)))))
def _estimate_normals(ctx, a, m, env):
    return ctx.estimate_normals(list(a["slots"]), k=a["k"], curvature=True)


# ---- mutators: filters (src -> dst; dst may be src)

def _filter_legal(min_points=3, normals=False):
    def legal(m, a):
        return _first(_slot_ok(a["dst"]), _slot_ok(a["src"]), _atleast(m, a["src"], min_points), _clean(m, a["src"]),
                      _has_normals(m, a["src"]) if normals else None)
    return legal


def _filter_draw(params):
    def draw(m, rng):
        s = _pick(rng, _nonempty(m, 3, clean=True))
        if s is None:
            return None
        a = dict(dst=_pick(rng, (s, FILTER_DST) + CLOUD_SLOTS), src=s)
        a.update(params(m[s].n, rng))
        return a
    return draw


def _filter(name, params, **kw):
    return _op(name, "mutator", dst_role="dst", src_role="src", reads=lambda a: (a["src"],), writes=lambda a: (a["dst"],), legal=_filter_legal(**kw),
               draw=_filter_draw(params))


@_op("denoise", "mutator", dst_role="slot", reads=lambda a: (a["slot"],), writes=lambda a: (a["slot"],),
     legal=lambda m, a: _first(_slot_ok(a["slot"]), _atleast(m, a["slot"], 3), _clean(m, a["slot"])),
     draw=lambda m, rng: (lambda s: s is not None and dict(slot=s, threshold=4, length=round(2.5 * spacing(m[s].n), 3)) or None)(
         _pick(rng, _nonempty(m, 3, clean=True))))
def _denoise(ctx, a, m, env):
    return ctx.denoise(a["slot"], a["threshold"], a["length"])


@_filter("voxel_grid", lambda n, rng: dict(leaf=round(2.0 * spacing(n), 3)))
def _voxel_grid(ctx, a, m, env):
    return ctx.voxel_grid(a["dst"], a["src"], a["leaf"], return_map=True)


@_filter("statistical_outlier_removal", lambda n, rng: dict(mean_k=8, mul=1.0))
def _sor(ctx, a, m, env):
    return ctx.statistical_outlier_removal(a["dst"], a["src"], a["mean_k"], a["mul"], return_index=True, return_dist=True, return_stats=True)


@_filter("radius_outlier_removal", lambda n, rng: dict(radius=round(1.5 * spacing(n), 3), min_neighbors=4))
def _ror(ctx, a, m, env):
    return ctx.radius_outlier_removal(a["dst"], a["src"], a["radius"], a["min_neighbors"], return_index=True, return_counts=True)


@_filter("extract_indices", lambda n, rng: dict(stride=int(_pick(rng, (2, 3, 7))), negative=bool(rng.integers(0, 2))))
def _extract_indices(ctx, a, m, env):
    return ctx.extract_indices(a["dst"], a["src"], np.arange(0, m[a["src"]].n, a["stride"], dtype=np.uint32), negative=a["negative"])


@_filter("segment_plane", lambda n, rng: dict(threshold=round(0.5 * spacing(n), 3), seed=int(rng.integers(1, 5)), negative=bool(rng.integers(0, 2))))
def _segment_plane(ctx, a, m, env):
    return ctx.segment_plane(a["dst"], a["src"], a["threshold"], max_iterations=50, seed=a["seed"], negative=a["negative"], return_index=True)


@_filter("mls", lambda n, rng: dict(radius=round(3.0 * spacing(n), 3), compute_normals=bool(rng.integers(0, 2))))
def _mls(ctx, a, m, env):
    return ctx.mls(a["dst"], a["src"], a["radius"], compute_normals=a["compute_normals"], return_index=True, return_curvature=True)


@_filter("iss_keypoints", lambda n, rng: dict(salient=round(4.0 * spacing(n), 3), non_max=round(3.0 * spacing(n), 3)))
def _iss(ctx, a, m, env):
    return ctx.iss_keypoints(a["dst"], a["src"], a["salient"], a["non_max"], return_index=True, return_saliency=True)


# ---- mutators: aligns (out: another slot, the source itself, or -1)

def _align_legal(normals=False):
    def legal(m, a):
        s, t, o = a["src"], a["tgt"], a["out"]
        return _first(_slot_ok(s), _slot_ok(t), None if o == -1 else _slot_ok(o), "src == tgt" if s == t else None,
                      "out == tgt" if o == t else None, _atleast(m, s, 3), _atleast(m, t, 3), _clean(m, s, t),
                      _has_normals(m, s, t) if normals else None)
    return legal


def _align_draw(normals=False, **fixed):
    def draw(m, rng):
        c = _nonempty(m, 3, clean=True, normals=normals)
        if len(c) < 2:
            return None
        s, t = (int(x) for x in rng.permutation(c)[:2])
        out = _pick(rng, [s, -1] + [x for x in CLOUD_SLOTS if x != t])
        a = dict(src=s, tgt=t, out=int(out), max_iter=int(_pick(rng, (1, 3, 10))), max_dist=max(4.0, round(2.0 * spacing(m[s].n), 3)))
        a.update(fixed)
        return a
    return draw


def _align(name, normals=False):
    return _op(name, "mutator", dst_role="out", src_role="src", reads=lambda a: (a["src"], a["tgt"]), writes=lambda a: () if a["out"] < 0 else (a["out"],),
               legal=_align_legal(normals), draw=_align_draw(normals))


def _icp_params(env, a, reciprocal=True):
    # max_iter 1: the reference's settings (one iteration and done); more: every convergence test but the iteration count off
    if a["max_iter"] == 1:
        return env.mvr.icp_params(reciprocal=reciprocal, max_dist=a["max_dist"], max_iter=1000)
    return env.mvr.icp_params(reciprocal=reciprocal, max_dist=a["max_dist"], max_iter=a["max_iter"], teps=0.0, feps=-1e300)


@_align("icp_align")
def _icp_align(ctx, a, m, env):
    return ctx.icp_align(a["src"], a["tgt"], a["out"], _icp_params(env, a))


@_align("icp_align_rejected")
def _icp_align_rejected(ctx, a, m, env):
    chain = [env.mvr.rejector("one_to_one"), env.mvr.rejector("median", 2.0)]      # one_to_one: the winner table is used
    return ctx.icp_align_rejected(a["src"], a["tgt"], a["out"], _icp_params(env, a, reciprocal=False), chain, return_trace=True)


@_align("icp_align_gicp", normals=True)
def _icp_align_gicp(ctx, a, m, env):
    p = env.mvr.gicp_params(max_corr_dist=a["max_dist"], max_iterations=min(a["max_iter"], 3))
    return ctx.icp_align_gicp(a["src"], a["tgt"], a["out"], p, return_trace=True)


def _prerej_legal(m, a):
    s, t = a["src"], a["tgt"]
    return _first(_slot_ok(s), _slot_ok(t), "src == tgt" if s == t else None, _atleast(m, s, 65), _atleast(m, t, 65), _clean(m, s, t),
                  _has_normals(m, s, t))


def _prerej_draw(m, rng):
    c = _nonempty(m, 65, clean=True, normals=True)
    if len(c) < 2:
        return None
    s, t = (int(x) for x in rng.permutation(c)[:2])
    return dict(src=s, tgt=t, radius=round(5.0 * spacing(min(m[s].n, m[t].n)), 3), seed=int(rng.integers(1, 9)))


@_op("align_prerejective", "mutator", src_role="src", reads=lambda a: (a["src"], a["tgt"]), writes=lambda a: (), legal=_prerej_legal, draw=_prerej_draw)
def _align_prerejective(ctx, a, m, env):
    sf, tf = ctx.fpfh(a["src"], a["radius"]), ctx.fpfh(a["tgt"], a["radius"])
    return sf, tf, ctx.align_prerejective(a["src"], a["tgt"], sf, tf, max_iterations=40, max_dist=a["radius"], inlier_fraction=0.1, seed=a["seed"])


# ---- mutators: the two drivers

def _ring_legal(m, a):
    posed, raw = a["posed"], a["raw"]
    if len(posed) != len(raw) or len(raw) < 2 or len(set(posed) | set(raw)) != 2 * len(raw):
        return "V distinct posed and V distinct raw slots"
    for s in posed:
        if _slot_ok(s):
            return _slot_ok(s)
    for s in raw:
        r = _first(_slot_ok(s), _atleast(m, s, 3), _clean(m, s), _plain(m, s, "raw slot"), "raw slot %d has normals" % s if m[s].nrm is not None else None)
        if r:
            return r
    return None


def _ring_draw(m, rng):
    raw = [s for s in _nonempty(m, 65, clean=True, plain=True) if m[s].nrm is None]
    if len(raw) < 2:
        return None
    raw = [int(s) for s in rng.permutation(raw)[:3]]
    posed = [int(s) for s in rng.permutation([s for s in CLOUD_SLOTS if s not in raw])[:len(raw)]]
    if len(posed) != len(raw):
        return None
    return dict(posed=posed, raw=raw, pose=[_pick(rng, ("eye",) + POSES) for _ in raw], max_dist=max(4.0, round(2.0 * spacing(min(m[s].n for s in raw)), 3)))


@_op("ring_step", "mutator", dst_role="posed", src_role="raw", reads=lambda a: tuple(a["raw"]), writes=lambda a: tuple(a["posed"]), legal=_ring_legal, draw=_ring_draw)
def _ring_step(ctx, a, m, env):
    V = len(a["raw"])
    edges = [(v, (v + 1) % V) for v in range(V)] if V > 2 else [(0, 1), (1, 0)]
    return ctx.ring_step(a["posed"], a["raw"], edges, [env.pose(p) for p in a["pose"]], a["max_dist"], np.array(env.pivot))


def _seq_legal(m, a):
    raw, three = a["raw"], (a["target"], a["source"], a["out"])
    if len(raw) < 2 or len(set(raw) | set(three)) != len(raw) + 3:
        return "distinct raw, target, source and out slots"
    for s in three:
        if _slot_ok(s):
            return _slot_ok(s)
    for s in raw:
        r = _first(_slot_ok(s), _atleast(m, s, 3), _clean(m, s), _plain(m, s, "raw slot"), "raw slot %d has normals" % s if m[s].nrm is not None else None)
        if r:
            return r
    return None if sum(m[s].n for s in raw) <= MAX_POINTS else "the model would grow beyond MAX_POINTS"


def _seq_draw(m, rng):
    raw = [s for s in _nonempty(m, 65, clean=True, plain=True) if m[s].nrm is None]
    raw = [int(s) for s in rng.permutation(raw)[:3]]
    rest = [int(s) for s in rng.permutation([s for s in CLOUD_SLOTS if s not in raw])]
    if len(raw) < 2 or len(rest) < 3 or sum(m[s].n for s in raw) > MAX_POINTS:
        return None
    return dict(raw=raw, target=rest[0], source=rest[1], out=rest[2], pose=[_pick(rng, ("eye",) + POSES) for _ in raw],
                max_dist=max(4.0, round(2.0 * spacing(min(m[s].n for s in raw)), 3)))


@_op("seq_run", "mutator", dst_role="target", src_role="raw", reads=lambda a: tuple(a["raw"]), writes=lambda a: (a["target"], a["source"], a["out"]), legal=_seq_legal, draw=_seq_draw)
def _seq_run(ctx, a, m, env):
    return ctx.seq_run(a["raw"], a["target"], a["source"], a["out"], env.mvr.icp_params(max_dist=a["max_dist"], max_iter=1000),
                       [env.pose(p) for p in a["pose"]])


# ---- cache builders (write no slot)

def _pair_legal(m, a, k=1):
    s, t = a["src"], a["tgt"]
    return _first(_slot_ok(s), _slot_ok(t), _atleast(m, s, k), _atleast(m, t, k), _clean(m, s, t))


def _pair_draw(**fixed):
    def draw(m, rng):
        c = _nonempty(m, 1, clean=True)
        if not c:
            return None
        a = dict(src=int(_pick(rng, c + [8])), tgt=int(_pick(rng, c)))
        a.update({k: (_pick(rng, v) if isinstance(v, tuple) else v) for k, v in fixed.items()})
        return a
    return draw


def _builder(name, draw, legal=_pair_legal):
    return _op(name, "builder", reads=lambda a: (a["src"], a["tgt"]), writes=lambda a: (), legal=legal, draw=draw)


@_builder("nn", _pair_draw())
def _nn(ctx, a, m, env):
    return ctx.nn(a["src"], a["tgt"])


@_builder("knn", _pair_draw(k=(1, 9, 17)), legal=lambda m, a: _first(_slot_ok(a["src"]), _slot_ok(a["tgt"]), _atleast(m, a["tgt"], 1), _clean(m, a["src"])))
def _knn(ctx, a, m, env):
    return ctx.knn(a["src"], a["tgt"], a["k"])


@_builder("correspondences", _pair_draw(reciprocal=(True, False)))
def _correspondences(ctx, a, m, env):
    return ctx.correspondences(a["src"], a["tgt"], CORR_DIST, reciprocal=a["reciprocal"])


@_builder("pair_moments2", _pair_draw())
def _pair_moments2(ctx, a, m, env):
    return ctx.pair_moments2(a["src"], a["tgt"], CORR_DIST, np.array(env.pivot))


def _pmb_draw(m, rng):
    c = _nonempty(m, 3, clean=True)
    if len(c) < 2:
        return None
    c = [int(s) for s in rng.permutation(c)[:3]]
    return dict(pairs=[[c[k], c[(k + 1) % len(c)]] for k in range(len(c))])


@_op("pair_moments2_batch", "builder", reads=lambda a: tuple(s for p in a["pairs"] for s in p), writes=lambda a: (),
     legal=lambda m, a: _first(*[_first(_pair_legal(m, dict(src=p[0], tgt=p[1]), 3), "src == tgt" if p[0] == p[1] else None) for p in a["pairs"]]), draw=_pmb_draw)
def _pair_moments2_batch(ctx, a, m, env):
    return ctx.pair_moments2_batch([tuple(p) for p in a["pairs"]], CORR_DIST, np.array(env.pivot))


def _self_draw(m, rng):
    s = _pick(rng, _nonempty(m, 3, clean=True, normals=True))
    return None if s is None else dict(slot=int(s), radius=round(3.0 * spacing(m[s].n), 3))


def _self_legal(m, a):
    return _first(_slot_ok(a["slot"]), _atleast(m, a["slot"], 3), _clean(m, a["slot"]), _has_normals(m, a["slot"]))


@_op("fpfh", "builder", reads=lambda a: (a["slot"],), writes=lambda a: (), legal=_self_legal, draw=_self_draw)
def _fpfh(ctx, a, m, env):
    return ctx.fpfh(a["slot"], a["radius"], return_counts=True)


@_op("boundary", "builder", reads=lambda a: (a["slot"],), writes=lambda a: (), legal=_self_legal, draw=_self_draw)
def _boundary(ctx, a, m, env):
    return ctx.boundary(a["slot"], a["radius"], return_gap=True, return_counts=True)


@_builder("pose_scores", _pair_draw(), legal=lambda m, a: _pair_legal(m, a, 3))
def _pose_scores(ctx, a, m, env):
    return ctx.pose_scores(a["src"], a["tgt"], np.stack([env.pose(p) for p in ("eye",) + POSES]), CORR_DIST)


@_builder("fitness", _pair_draw(pose=POSES))
def _fitness(ctx, a, m, env):
    return ctx.fitness(a["src"], a["tgt"], env.pose(a.get("pose", "nudge")))


def _probe_ok(m, a):
    return all(m[s].n >= 3 and not m[s].dirty for s in (a["slot"], a["other"]))


@_op("probe", "builder", reads=lambda a: (a["slot"], a["other"]), writes=lambda a: (),
     legal=lambda m, a: _first(_slot_ok(a["slot"]), _slot_ok(a["other"]), "slot == other" if a["slot"] == a["other"] else None), draw=lambda m, rng: None)
def _probe(ctx, a, m, env):
    """consumes the state that no search reads -- the aligns' seeds, the winner table, the fused batch's pair records -- with the
    slot as source and as target; nothing where a slot holds fewer than 3 points"""
    if not _probe_ok(m, a):
        return None
    s, o = a["slot"], a["other"]
    p = env.mvr.icp_params(max_dist=4.0, max_iter=1000)
    chain = [env.mvr.rejector("one_to_one")]
    return (ctx.icp_align(s, o, -1, p), ctx.icp_align(o, s, -1, p), ctx.icp_align_rejected(s, o, -1, env.mvr.icp_params(reciprocal=False, max_dist=4.0, max_iter=1000), chain),
            ctx.pair_moments2_batch([(s, o), (o, s)], CORR_DIST, np.array(env.pivot)))


MUTATORS = tuple(n for n, o in OPS.items() if o.kind == "mutator")
BUILDERS = tuple(n for n, o in OPS.items() if o.kind == "builder" and n != "probe")
ALIGNS = ("icp_align", "icp_align_rejected", "icp_align_gicp")
POINT_PRESERVING = ("reserve", "set_global_base", "upload_normals", "estimate_normals")      # mutators that leave the points as they are
NO_OUTPUT_SLOT = ("align_prerejective",)                                                      # writes the context's scratch clouds only


# ------------------------------------------------------------------ the bookkeeping rules (DESIGN.md's table, executable)

# per writing entry, what the DESTINATION keeps of: point-set id, ordering, pose/canonical, set grid, model grid, normals,
# segments.  'new' a new id / canonical again, 'src' taken from the source, 'keep', 'drop', 'extend' (the old ordering grown by
# the source's where both exist and the old one is not shared, else dropped), 'posed' (a known pose of the source's set where
# the source was canonical and the matrix is rigid to 1e-3), 'rot' normals rotated with the points, 'follow' the kept points'
# normals, 'set' written by the call, 'both' kept where both parts have them, 'push' one more segment where it is a shard.
COLUMNS = ("set id", "ordering", "pose", "set grid", "model grid", "normals", "segments")
KEEPS = {
    "upload":                        ("new", "drop", "canonical", "drop", "drop", "drop", "drop"),
    "clear":                         ("new", "drop", "canonical", "drop", "drop", "drop", "drop"),
    "reserve":                       ("keep", "keep", "keep", "keep", "keep", "keep", "keep"),
    "copy":                          ("src", "src", "src", "src", "drop", "src", "src"),
    "append":                        ("new", "extend", "canonical", "drop", "drop", "both", "push"),
    "set_global_base":               ("keep", "keep", "keep", "keep", "keep", "keep", "set"),
    "append_range":                  ("new", "drop", "canonical", "drop", "drop", "drop", "push"),
    "transform":                     ("src", "src", "posed", "src if posed", "drop", "rot", "src"),
    "transform (in place)":          ("keep", "keep", "drop", "drop", "drop", "rot", "keep"),
    "transform_f32":                 ("src", "src", "drop", "drop", "drop", "rot", "src"),
    "transform_f32 (in place)":      ("keep", "keep", "drop", "drop", "drop", "rot", "keep"),
    "transform_batch":               ("src", "src", "posed", "src if posed", "drop", "rot", "src"),
    "transform_batch (in place)":    ("keep", "keep", "drop", "drop", "drop", "rot", "keep"),
    "upload_normals":                ("keep", "keep", "keep", "keep", "keep", "set", "keep"),
    "estimate_normals":              ("keep", "keep", "keep", "keep", "keep", "set", "keep"),
    "denoise":                       ("new", "drop", "canonical", "drop", "drop", "follow", "drop"),
    "voxel_grid":                    ("new", "drop", "canonical", "drop", "drop", "follow", "drop"),
    "statistical_outlier_removal":   ("new", "drop", "canonical", "drop", "drop", "follow", "drop"),
    "radius_outlier_removal":        ("new", "drop", "canonical", "drop", "drop", "follow", "drop"),
    "extract_indices":               ("new", "drop", "canonical", "drop", "drop", "follow", "drop"),
    "segment_plane":                 ("new", "drop", "canonical", "drop", "drop", "follow", "drop"),
    "mls":                           ("new", "drop", "canonical", "drop", "drop", "follow or set", "drop"),
    "iss_keypoints":                 ("new", "drop", "canonical", "drop", "drop", "follow", "drop"),
    "icp_align":                     ("src", "src", "drop", "drop", "drop", "rot", "src"),
    "icp_align (in place)":          ("keep", "keep", "drop", "drop", "drop", "rot", "keep"),
    "icp_align_rejected":            ("src", "src", "drop", "drop", "drop", "rot", "src"),
    "icp_align_rejected (in place)": ("keep", "keep", "drop", "drop", "drop", "rot", "keep"),
    "icp_align_gicp":                ("src", "src", "drop", "drop", "drop", "rot", "src"),
    "icp_align_gicp (in place)":     ("keep", "keep", "drop", "drop", "drop", "rot", "keep"),
    "align_prerejective":            ("-", "-", "-", "-", "-", "-", "-"),
    "ring_step":                     ("src", "src", "posed", "src if posed", "drop", "rot", "src"),
    "seq_run":                       ("as its transforms, aligns and appends",) * 7,
}


def segs_after(name, a, pre, slot):
    """the segment table of written slot `slot` after the call (pre: the model before it)"""
    if name in ("reserve", "upload_normals", "estimate_normals"):
        return list(pre[slot].segs)
    if name == "set_global_base":
        return [(0, pre[slot].n, a["base"])]
    if name == "append":
        d, s = pre[a["dst"]], pre[a["src"]]
        gend = max([gb + cnt for _, cnt, gb in d.segs], default=0)
        return d.segs + [(d.n, s.n, gend)] if d.segs else []
    if name == "append_range":
        d = pre[a["dst"]]
        return (d.segs or ([(0, d.n, 0)] if d.n else [])) + [(d.n, a["count"], a["base"])]
    if name in ("copy", "transform", "transform_f32") + ALIGNS:
        dst = a["out"] if name in ALIGNS else a["dst"]
        return list(pre[a["src"] if dst != a["src"] else dst].segs)
    if name == "transform_batch":
        k = a["dst"].index(slot)
        return list(pre[a["src"][k]].segs)
    return []          # upload, clear, every filter, ring_step and seq_run (their raw slots are plain)


def normals_after(name, a, pre, slot, n_out):
    """True / False: whether written slot `slot` (n_out points now) has normals after the call; None: not predicted"""
    def has(s):
        return pre[s].nrm is not None
    if n_out == 0 or name in ("upload", "clear", "append_range"):
        return False
    if name in ("reserve", "set_global_base", "denoise"):
        return has(slot)
    if name in ("upload_normals", "estimate_normals"):
        return True
    if name == "append":
        d, s = a["dst"], a["src"]
        return has(d) if pre[s].n == 0 else has(s) and (has(d) or pre[d].n == 0)
    if name == "transform_batch":
        return has(a["src"][a["dst"].index(slot)])
    if name == "ring_step":
        return has(a["raw"][a["posed"].index(slot)])
    if name == "mls":
        return a["compute_normals"] or has(a["src"])
    if name == "seq_run":
        return False
    return has(a["src"])


def dirty_after(name, a, pre, slot, env):
    if name == "upload":
        return a["cloud"].startswith("dirty")
    if name == "clear":
        return False
    if name in ("append", "append_range"):
        return pre[a["dst"]].dirty or pre[a["src"]].dirty
    if name == "copy":
        return pre[a["src"]].dirty
    return pre[slot].dirty if name in POINT_PRESERVING else False


# ------------------------------------------------------------------ comparing results bit for bit

def canon(x):
    """a result in a form that == compares bit for bit (NaN == NaN, -0.0 != 0.0), VOLATILE keys left out"""
    if x is None or isinstance(x, (bool, int, str, bytes)):
        return x
    if isinstance(x, float):
        return ("f64", struct.pack("<d", x))
    if isinstance(x, np.generic):
        return canon(x.item()) if not isinstance(x, np.floating) else (str(x.dtype), x.tobytes())
    if isinstance(x, np.ndarray):
        return (str(x.dtype), x.shape, np.ascontiguousarray(x).tobytes())
    if isinstance(x, (ctypes.Structure, ctypes.Array)):
        return ("ctypes", bytes(x))
    if isinstance(x, dict):
        return tuple((k, canon(v)) for k, v in sorted(x.items()) if k not in VOLATILE)
    if isinstance(x, (list, tuple)):
        return tuple(canon(v) for v in x)
    raise TypeError("canon: %r" % type(x))


def where_differs(a, b, path="result"):
    """the first place two canonical results differ, for the failure message"""
    if type(a) is not type(b):
        return "%s: %s != %s" % (path, type(a).__name__, type(b).__name__)
    if isinstance(a, tuple):
        if len(a) == 3 and isinstance(a[2], bytes) and isinstance(a[0], str):
            return None if a == b else "%s: arrays %s %s / %s %s differ" % (path, a[0], a[1], b[0], b[1])
        if len(a) != len(b):
            return "%s: %d != %d entries" % (path, len(a), len(b))
        for k, (u, v) in enumerate(zip(a, b)):
            d = where_differs(u, v, "%s[%s]" % (path, u[0] if isinstance(u, tuple) and len(u) == 2 and isinstance(u[0], str) else k))
            if d:
                return d
        return None
    return None if a == b else "%s: %r != %r" % (path, a, b)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def fmt(seq):
    """a sequence as text that can be pasted back as a scenario"""
    return "[\n" + "".join("    (%r, %r),\n" % (n, a) for n, a in seq) + "]"


class CheckFailure(AssertionError):
    def __init__(self, step, what, detail, seq):
        self.step, self.what, self.detail = step, what, detail
        name, a = seq[step]
        super().__init__("step %d (%s %r): %s: %s\nthe sequence up to it:\n%s" % (step, name, a, what, detail, fmt(seq[:step + 1])))


# ------------------------------------------------------------------ the checker

class Checker:
    """runs a sequence on one long-lived context (make_ctx()) and checks it after every step; make_ctx() also makes the clean
    rooms.  export_keys(ctx, s, t) -> int64 keys of nn_forward_keys (the caller knows how to hold a device buffer)."""

    def __init__(self, make_ctx, env, export_keys=None, clean_room=True, searches=True):
        self.make_ctx, self.env, self.export_keys, self.clean_room = make_ctx, env, export_keys, clean_room
        self.searches = searches              # False: no search after the steps (a mutator then meets slots without an ordering, a sorted copy or a grid), all of them after the last
        self.align_iterations, self.order_log, self.errors = [], [], []
        self.t_clean = 0.0

    # -- device <-> model
    def observe(self, ctx, s):
        pts = ctx.download(s)
        nrm = ctx.download_normals(s) if len(pts) else np.zeros((0, 4), F32)
        return pts, (nrm if len(pts) and len(nrm) == len(pts) else None)

    def stage(self, ctx, s, sl):
        """slot s of a fresh context <- the model's copy: points, the segment table, normals"""
        if isinstance(sl.recipe, dict) and len(sl.segs) <= 1 and hasattr(ctx, "debug_order") and self.build(ctx, s, sl.recipe, 0) and same(ctx.download(s), sl.pts):
            if sl.segs:
                ctx.set_global_base(s, sl.segs[0][2])
        elif not sl.segs:
            ctx.upload(s, sl.pts)
        else:
            ctx.clear(s)
            for lb, cnt, gb in sl.segs:
                ctx.upload(STAGE, sl.pts[lb:lb + cnt])
                ctx.append_range(s, STAGE, 0, cnt, gb)
        if sl.nrm is not None:
            ctx.upload_normals(s, sl.nrm)

    def build(self, ctx, s, rec, cap):
        """slot s <- the points of a recipe with the ordering built the way the recipe says"""
        if not isinstance(rec, dict):
            return False
        if rec["kind"] == "via":
            ctx.upload(s, rec["pts"])
            getattr(ctx, rec["fn"])(STAGE + 1, s, rec["T"])
        elif rec["kind"] == "base":
            if cap:
                ctx.reserve(s, cap)
            ctx.upload(s, rec["pts"])
            if len(rec["pts"]):
                ctx.nn(s, s)
        else:
            if not (isinstance(rec["a"], dict) and isinstance(rec["b"], dict)):
                return False
            if not self.build(ctx, s, rec["a"], max(cap, rec["n"])) or not self.build(ctx, STAGE + 1, rec["b"], 0):
                return False
            ctx.append(s, STAGE + 1)
        for fn, T in rec["chain"]:
            getattr(ctx, fn)(s, s, T)
        return True

    def track(self, name, a, pre, res, written):
        """the recipes of the written slots after the call (the library's rules for who inherits whose ordering)"""
        ctx, env, m = self.ctx, self.env, self.model

        def has(s):
            return ctx.debug_order(s) is not None
        moves = []
        if name == "copy":
            moves = [(a["dst"], a["src"], None, None)]
        elif name in ("transform", "transform_f32"):
            moves = [(a["dst"], a["src"], name, env.pose(a["pose"]))]
        elif name == "transform_batch":
            moves = [(d, s_, "transform", env.pose(p_)) for d, s_, p_ in zip(a["dst"], a["src"], a["pose"])]
        elif name == "ring_step":
            moves = [(d, s_, "transform", env.pose(p_)) for d, s_, p_ in zip(a["posed"], a["raw"], a["pose"])]
        elif name in ALIGNS and a["out"] >= 0:
            moves = [(a["out"], a["src"], "transform_f32", np.array(res[0]))]
        new = {s: (pre[s].recipe if name in POINT_PRESERVING else "unknown" if name == "seq_run" else None) for s in written}
        for d, src, fn, T in moves:
            rs = pre[src].recipe
            if d != src and rs is None and has(src) and name in ALIGNS:      # the align ordered its source first, from the points it has
                rs = m[src].recipe = dict(kind="base", pts=pre[src].pts, chain=[])
            elif d != src and rs is None and has(src):
                # a posed copy of a cloud that was never searched: the SET's ordering is built from the posed points and the source
                # shares it -- the source came by its ordering through this very call, and the copy's is that of its own points
                m[src].recipe = dict(kind="via", pts=pre[src].pts, fn=fn, T=T, chain=[])
            new[d] = dict(rs, chain=rs["chain"] + [(fn, T)]) if isinstance(rs, dict) and fn else rs
        if name == "append":
            d, src = a["dst"], a["src"]
            if pre[src].n == 0:
                new[d] = pre[d].recipe
            elif d != src and pre[d].n and has(d):            # the ordering is there without a search: extended
                ok = isinstance(pre[d].recipe, dict) and isinstance(pre[src].recipe, dict)
                new[d] = dict(kind="append", a=pre[d].recipe, b=pre[src].recipe, n=pre[d].n + pre[src].n, chain=[]) if ok else "unknown"
        for s in written:
            m[s].recipe = new[s]

    def run(self, seq):
        self.seq = list(seq)
        self.model = Model()
        self.ctx = self.make_ctx()
        try:
            for k, (name, a) in enumerate(self.seq):
                self.step(k, name, a)
            if not self.searches:
                for s in WORKING:
                    self.search(len(self.seq) - 1, s)
            self.finish(self.ctx)
        finally:
            self.ctx.close()
        return self

    def run_random(self, seed, steps=None, prologue=None):
        """a seeded random sequence, drawn step by step against the model as the context under test leaves it (what a filter
        keeps decides which calls are legal after it); self.seq is the plain list that was run"""
        rng = np.random.default_rng(seed)
        self.seq = []
        self.model = Model()
        self.ctx = self.make_ctx()
        names = sorted(OPS)
        prologue = RANDOM_PROLOGUE if prologue is None else prologue
        try:
            for name, a in prologue:
                self.seq.append((name, a))
                self.step(len(self.seq) - 1, name, a)
            while len(self.seq) < len(prologue) + (steps or RANDOM_STEPS):
                name = names[int(rng.integers(0, len(names)))]
                a = OPS[name].draw(self.model, rng)
                if not a or OPS[name].legal(self.model, a) is not None:
                    continue
                # (a call whose sums follow the ordering of a slot that the clean room cannot rebuild -- seq_run's model and scans, an
                # extension of one -- could only be compared by tolerance: not drawn)
                if name in ORDER_SENSITIVE and any(self.model[x].recipe == "unknown" for x in OPS[name].reads(a)):
                    continue
                self.seq.append((name, a))
                self.step(len(self.seq) - 1, name, a)
            self.finish(self.ctx)
        finally:
            self.ctx.close()
        return self

    def finish(self, ctx):
        """hook: read the long-lived context's counters before it closes"""

    def before_step(self, k, ctx):
        """hook"""

    def fail(self, k, what, detail=""):
        raise CheckFailure(k, what, detail, self.seq)

    def step(self, k, name, a):
        import time
        op, env, ctx, pre = OPS[name], self.env, self.ctx, self.model.snapshot()
        why = op.legal(pre, a)
        if why:
            self.fail(k, "illegal call", why)
        written = tuple(dict.fromkeys(op.writes(a)))
        self.before_step(k, ctx)
        order_before = ctx.debug_order(a["dst"]) if name == "append" and hasattr(ctx, "debug_order") else None
        res = op.run(ctx, a, pre, env)
        if name == "append" and hasattr(ctx, "debug_order"):
            self.order_log.append((k, order_before, ctx.debug_order(a["dst"])))
        if name in ALIGNS:
            self.align_iterations.append(res[1]["iterations"])
        # -- the model takes what the device returned; the slots the call did not write are bit-unchanged
        for s in WORKING:
            pts, nrm = self.observe(ctx, s)
            if s in written:
                want = normals_after(name, a, pre, s, len(pts))
                if want is not None and want != (nrm is not None):
                    self.fail(k, "normals of slot %d" % s, "the slot %s normals, the rule says it %s" % (("has", "has none") if nrm is not None else ("has no", "has them")))
                self.model.slots[s] = Slot(pts, nrm, segs_after(name, a, pre, s), dirty_after(name, a, pre, s, env))
            elif not same(pts, pre[s].pts) or (nrm is None) != (pre[s].nrm is None) or (nrm is not None and not same(nrm, pre[s].nrm)):
                self.fail(k, "untouched slot %d changed" % s, "%d points before, %d after" % (pre[s].n, len(pts)))
        tracking = hasattr(ctx, "debug_order")
        if tracking:
            self.track(name, a, pre, res, written)
        # -- clean room
        if self.clean_room:
            t0 = time.perf_counter()
            fresh = self.make_ctx(clean=True)
            try:
                for s in dict.fromkeys(tuple(op.reads(a)) + written):
                    self.stage(fresh, s, pre[s])
                res2 = op.run(fresh, a, pre, env)
                d = where_differs(canon(res), canon(res2))
                if d:
                    if tracking:      # which of the slots the call read is ordered differently here and there, and how the model thought it came by its ordering
                        for x in dict.fromkeys(op.reads(a)):
                            o1, o2 = ctx.debug_order(x), fresh.debug_order(x)
                            if (o1 is None) != (o2 is None) or (o1 is not None and not np.array_equal(o1, o2)):
                                r = pre[x].recipe
                                d += "; the ordering of slot %d differs (recipe: %s)" % (x, r if not isinstance(r, dict) else (r["kind"], [f for f, _ in r["chain"]]))
                    self.fail(k, "clean room: return values differ", d[-700:] if len(d) > 900 else d)
                for s in written:
                    pts, nrm = self.observe(fresh, s)
                    if not same(pts, self.model[s].pts):
                        self.fail(k, "clean room: points of slot %d differ" % s, "%d here, %d in the fresh context" % (self.model[s].n, len(pts)))
                    if (nrm is None) != (self.model[s].nrm is None) or (nrm is not None and not same(nrm, self.model[s].nrm)):
                        self.fail(k, "clean room: normals of slot %d differ" % s)
            finally:
                fresh.close()
            self.t_clean += time.perf_counter() - t0
        # -- searches over what the step touched and one slot it did not
        touched = [s for s in dict.fromkeys(tuple(op.reads(a)) + written) if s in WORKING]
        others = [s for s in CLOUD_SLOTS if s not in touched and self.model[s].n]
        if others:
            touched.append(others[k % len(others)])
        if self.searches:
            for s in touched:
                self.search(k, s)
        if tracking:                          # an ordering that was built in this step was built from the points as they are now
            for s in WORKING:
                if self.model[s].recipe is None and self.model[s].n and ctx.debug_order(s) is not None:
                    self.model[s].recipe = dict(kind="base", pts=self.model[s].pts, chain=[])

    # -- searches against the independent references
    def search(self, k, s):
        ctx, env, m = self.ctx, self.env, self.model
        P = m[s].pts
        if ctx.size(s) != len(P):
            self.fail(k, "search: size of slot %d" % s, "%d, the model holds %d" % (ctx.size(s), len(P)))
        qs, other = (8, 9) if s not in QUERY_SLOTS else ((9, 9) if s == 8 else (8, 8))
        Q = m[qs].pts
        if len(Q) == 0:
            return
        if len(P) == 0:
            i, d = ctx.nn(qs, s)
            if not (np.all(i == NONE) and np.all(np.isinf(d))):
                self.fail(k, "search: nn in the empty slot %d" % s, "found neighbours")
            return
        if not m[s].dirty:
            oi, od = env.ref(("nn",), (Q, P), lambda: env.orc.nn(Q, P, kdtree=len(P) > 2000))
            i, d = ctx.nn(qs, s)
            if not (np.array_equal(i, oi) and same(d, od)):
                self.fail(k, "search: nn(%d -> %d)" % (qs, s), "%d of %d indices differ from the oracle's" % (int((i != oi).sum()), len(oi)))
            R = m[other].pts
            if s not in QUERY_SLOTS and len(R):
                oi, od = env.ref(("nn",), (P, R), lambda: env.orc.nn(P, R, kdtree=len(R) > 2000))
                i, d = ctx.nn(s, other)
                if not (np.array_equal(i, oi) and same(d, od)):
                    self.fail(k, "search: nn(%d -> %d)" % (s, other), "%d of %d indices differ from the oracle's" % (int((i != oi).sum()), len(oi)))
            for rec in (True, False):
                c = env.ref(("corr", rec), (Q, P), lambda: env.orc.correspondences(Q, P, CORR_DIST, reciprocal=rec, kdtree=True))
                q_, m_, d_ = ctx.correspondences(qs, s, CORR_DIST, reciprocal=rec)
                if not (np.array_equal(q_, c["query"]) and np.array_equal(m_, c["match"]) and same(d_, np.ascontiguousarray(c["dist2"]))):
                    self.fail(k, "search: correspondences(%d -> %d, reciprocal=%s)" % (qs, s, rec), "%d here, %d in the oracle" % (len(q_), len(c)))
        ri, rd = env.ref(("knn",), (Q, P), lambda: N.knn_brute(Q, P, max(KNN_KS)))
        for kk in KNN_KS:                     # tests/test_gpu_walk_fuzz.py, check_knn: the list at a smaller k is the prefix
            gi, gd = ctx.knn(qs, s, kk)
            if not (np.array_equal(gi, ri[:, :kk]) and same(gd, rd[:, :kk])):
                self.fail(k, "search: knn(%d -> %d, k=%d)" % (qs, s, kk), "%d rows differ from knn_brute" % int((gi != ri[:, :kk]).any(axis=1).sum()))
        # the exported keys carry the model's global numbering: the table of a shard, the local index of a plain slot
        if self.export_keys and not m[s].dirty:
            keys = self.export_keys(ctx, qs, s)
            oi, od = env.ref(("nn-brute",), (Q, P), lambda: env.orc.nn(Q, P, kdtree=False))
            want = (bits(od).astype(np.int64) << 32) | m.global_index(s, oi)
            if not np.array_equal(keys, want):
                bad = np.nonzero(keys != want)[0]
                self.fail(k, "search: nn_forward_keys(%d -> %d)" % (qs, s), "%d of %d keys differ; first: local %d exported as %d, the model numbers it %d (table %r)"
                          % (len(bad), len(keys), oi[bad[0]], keys[bad[0]] & 0xFFFFFFFF, want[bad[0]] & 0xFFFFFFFF, m[s].segs))
        # the radius filter walks the slot's model grid; its output goes to the filter destination, which the model records
        r, mn = round(2.0 * spacing(len(P)), 3), 6          # (drops about a tenth of a synthetic view)
        ref = env.ref(("ror", r, mn, False), (P,), lambda: O.radius(P, r, mn))
        n_out, idx = ctx.radius_outlier_removal(FILTER_DST, s, r, mn, return_index=True)
        if not (n_out == len(ref["index"]) and np.array_equal(idx, ref["index"])):
            self.fail(k, "search: radius_outlier_removal(%d)" % s, "%d kept, outlier_ref.radius keeps %d" % (n_out, len(ref["index"])))
        pts, nrm = self.observe(ctx, FILTER_DST)
        src_nrm = m[s].nrm
        if not same(pts, P[idx]) or (nrm is not None) != (src_nrm is not None and n_out > 0) or (nrm is not None and not same(nrm, src_nrm[idx])):
            self.fail(k, "search: the filter destination after radius_outlier_removal(%d)" % s, "not the kept points and their normals")
        m.slots[FILTER_DST] = Slot(pts, nrm, [], m[s].dirty)


# ------------------------------------------------------------------ a numpy context with the same method names

class FakeContext:
    """The data-moving entries and the searches BY DEFINITION (numpy, brute force); every computing entry (filters other than
    the radius filter and extract_indices, normals, aligns, drivers, descriptors) as a STAND-IN: a deterministic function of
    the slots' contents that honours the entry's data contract -- which slots it reads and writes, whose normals follow --
    and nothing of its arithmetic, which the checker never predicts.  stale = (search, slot), settable at any time: that search
    answers for that target slot from its contents BEFORE its last mutation (what a stale index does); the checker must notice.
    align_keeps_table: an align leaves the segment table of its output slot alone (the library's rule before the aligns'
    output bookkeeping became finish_align_out); the checker's key comparison must notice that too."""

    def __init__(self, mvr=None, stale=None, ref=None, align_keeps_table=False):
        self.mvr, self.stale, self.align_keeps_table = mvr, stale, align_keeps_table
        self.ref = ref or (lambda tag, arrays, make: make())      # Env.ref: the radius filter's definition is slow, computed once per content
        self.s = {}
        self.prev = {}

    def close(self):
        pass

    def _get(self, s):
        return self.s.get(s) or Slot()

    def _set(self, s, pts, nrm=None, segs=()):
        self.prev[s] = self._get(s).pts
        pts = np.ascontiguousarray(pts, F32).reshape(-1, 4)
        self.s[s] = Slot(pts, None if nrm is None or not len(pts) else np.ascontiguousarray(nrm, F32), segs)

    def _target(self, s, search):
        return self.prev[s] if self.stale == (search, s) and s in self.prev else self._get(s).pts

    # -- clouds
    def upload(self, s, pts):
        p = np.ascontiguousarray(pts, F32)
        if p.shape[1] == 3:
            p = np.concatenate([p, np.ones((len(p), 1), F32)], axis=1)
        self._set(s, p.copy())

    def size(self, s):
        return self._get(s).n

    def download(self, s):
        return self._get(s).pts.copy()

    def upload_normals(self, s, nrm):
        assert len(nrm) == self.size(s)
        self._get(s).nrm = np.ascontiguousarray(nrm, F32).copy() if len(nrm) else None

    def download_normals(self, s):
        sl = self._get(s)
        return sl.nrm.copy() if sl.nrm is not None else np.zeros((0, 4), F32)

    def reserve(self, s, cap):
        self.s.setdefault(s, Slot())

    def clear(self, s):
        self._set(s, np.zeros((0, 4), F32))

    def copy(self, d, s):
        if d != s:
            sl = self._get(s)
            self._set(d, sl.pts.copy(), sl.nrm, list(sl.segs))

    def append(self, d, s):
        dl, sl = self._get(d), self._get(s)
        segs = list(dl.segs)
        if segs:
            segs.append((dl.n, sl.n, max(gb + c for _, c, gb in segs)))
        if sl.n == 0:
            dl.segs = segs
            self.s[d] = dl
            return
        keep = sl.nrm is not None and (dl.nrm is not None or dl.n == 0)
        nrm = np.concatenate([dl.nrm if dl.n else np.zeros((0, 4), F32), sl.nrm]) if keep else None
        self._set(d, np.concatenate([dl.pts, sl.pts]), nrm, segs)

    def set_global_base(self, s, base):
        self._get(s).segs = [(0, self.size(s), int(base))]

    def append_range(self, d, s, begin, count, base):
        assert d != s and begin + count <= self.size(s)
        dl = self._get(d)
        segs = list(dl.segs) or ([(0, dl.n, 0)] if dl.n else [])
        self._set(d, np.concatenate([dl.pts, self._get(s).pts[begin:begin + count]]), None, segs + [(dl.n, count, int(base))])

    @staticmethod
    def _move(pts, nrm, T, dtype):
        T = np.asarray(T, dtype)
        out = pts.copy()
        out[:, :3] = (pts[:, :3].astype(dtype) @ T[:3, :3].T + T[:3, 3]).astype(F32)
        n2 = None
        if nrm is not None:
            n2 = nrm.copy()
            n2[:, :3] = (nrm[:, :3].astype(dtype) @ T[:3, :3].T).astype(F32)
        return out, n2

    def transform(self, d, s, T, dtype=F64):
        sl = self._get(s)
        p, n = self._move(sl.pts, sl.nrm, T, dtype)
        self._set(d, p, n, list(sl.segs))

    def transform_f32(self, d, s, T):
        self.transform(d, s, T, F32)

    def transform_batch(self, ds, ss, Ts):
        for d, s, T in zip(ds, ss, Ts):
            self.transform(d, s, T)

    # -- searches, by definition
    @staticmethod
    def _nn(Q, P):
        i = np.full(len(Q), NONE, np.uint32)
        d = np.full(len(Q), np.inf, F32)
        if len(P) and len(Q):
            D = N.dist2_f32(Q, P)
            key = (D.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.arange(len(P), dtype=np.uint64)[None, :]
            best = key.min(axis=1)
            i, d = (best & np.uint64(0xFFFFFFFF)).astype(np.uint32), (best >> np.uint64(32)).astype(np.uint32).view(F32)
        return i, d

    def nn(self, q, t, fma=False):
        return self._nn(self._get(q).pts, self._target(t, "nn"))

    def knn(self, q, t, k, fma=False):
        return N.knn_brute(self._get(q).pts, self._target(t, "knn"), k)

    def correspondences(self, s, t, max_dist, reciprocal=True, fma=False):
        S, T = self._get(s).pts, self._target(t, "correspondences")
        j, d = self._nn(S, T)
        ok = (j != NONE) & (d.astype(F64) <= max_dist * max_dist)
        if reciprocal and len(T):
            back, db = self._nn(T, S)
            jj = np.where(ok, j, 0).astype(np.int64)
            ok &= (back[jj] == np.arange(len(S))) & (db[jj].astype(F64) <= max_dist * max_dist)
        q = np.nonzero(ok)[0]
        return q.astype(np.int32), j[q].astype(np.int32), d[q]

    def radius_outlier_removal(self, d, s, radius, min_neighbors, negative=False, fma=False, return_index=False, return_counts=False):
        sl = self._get(s)
        P = self._target(s, "radius")
        ref = self.ref(("ror", radius, min_neighbors, bool(negative)), (P,), lambda: O.radius(P, radius, min_neighbors, negative))
        idx = ref["index"]
        self._set(d, P[idx], sl.nrm[idx] if sl.nrm is not None and len(sl.nrm) == len(P) else None)
        out = [len(idx)] + ([idx] if return_index else []) + ([ref["count"]] if return_counts else [])
        return out[0] if len(out) == 1 else tuple(out)

    def extract_indices(self, d, s, index, negative=False):
        sl = self._get(s)
        keep = np.zeros(sl.n, bool)
        keep[np.asarray(index, np.int64)] = True
        idx = np.nonzero(~keep if negative else keep)[0]
        self._set(d, sl.pts[idx], sl.nrm[idx] if sl.nrm is not None else None)
        return len(idx)

    def fake_forward_keys(self, s, t):
        i, d = self._nn(self._get(s).pts, self._get(t).pts)
        m = Model()
        m.slots[0] = self._get(t)
        return (bits(d).astype(np.int64) << 32) | m.global_index(0, i)

    # -- stand-ins
    def _subset(self, d, s, keep, nrm="follow"):
        sl = self._get(s)
        idx = np.nonzero(keep)[0].astype(np.uint32)
        self._set(d, sl.pts[idx], sl.nrm[idx] if sl.nrm is not None else None)
        return idx

    def estimate_normals(self, slots, k=None, radius=None, curvature=False, **kw):
        sl = [slots] if np.isscalar(slots) else list(slots)
        for s in sl:
            self._get(s).nrm = model_normals(self._get(s).pts[:, [1, 2, 0, 3]])
        return [np.zeros(self.size(s), F32) for s in sl] if curvature else None

    def denoise(self, s, thr=10, length=2.5):
        return self._subset(s, s, np.arange(self.size(s)) % 7 != 3), 1

    def voxel_grid(self, d, s, leaf, min_points=0, return_map=False):
        sl = self._get(s)
        cell = np.floor(sl.pts[:, :3] / F32(leaf)).astype(np.int64)
        _, first, inv = np.unique(cell, axis=0, return_index=True, return_inverse=True)
        inv = inv.reshape(-1)
        out = np.zeros((len(first), 4), F64)
        np.add.at(out, inv, sl.pts.astype(F64))
        out /= np.bincount(inv, minlength=len(first))[:, None]
        self._set(d, out.astype(F32), sl.nrm[first] if sl.nrm is not None else None)
        return (len(first), inv.astype(np.uint32)) if return_map else len(first)

    def statistical_outlier_removal(self, d, s, mean_k, mul, return_index=False, return_dist=False, return_stats=False, **kw):
        n = self.size(s)
        idx = self._subset(d, s, np.arange(n) % 5 != 1)
        return len(idx), idx

    def mls(self, d, s, radius, compute_normals=False, return_index=False, return_curvature=False, **kw):
        sl = self._get(s)
        p = sl.pts.copy()
        p[:, :3] *= F32(1.0 + 2.0 ** -10)
        self._set(d, p, model_normals(p) if compute_normals else sl.nrm)
        return len(p), np.arange(len(p), dtype=np.uint32)

    def iss_keypoints(self, d, s, salient, non_max, return_index=False, return_saliency=False, **kw):
        idx = self._subset(d, s, np.arange(self.size(s)) % 4 == 0)
        return len(idx), idx

    def segment_plane(self, d, s, threshold, negative=False, return_index=False, **kw):
        keep = np.arange(self.size(s)) % 3 == 0
        idx = self._subset(d, s, ~keep if negative else keep)
        return dict(found=True, n_out=len(idx)), idx

    def _align_out(self, s, t, out, a=0.0):
        T = np.eye(4, dtype=F32)
        T[:3, 3] = (0.015625 * (1 + self.size(s) % 3), 0.0, -0.03125)
        if out >= 0:
            sl = self._get(s)
            p, n = self._move(sl.pts, sl.nrm, T, F32)
            self._set(out, p, n, list(self._get(out).segs if self.align_keeps_table and out != s else sl.segs))
        tp = self._target(t, "align")
        return T, dict(iterations=1 + self.size(t) % 2, converged=True, state="ITERATIONS", n_corr=int(np.abs(np.nan_to_num(tp[:, :3])).sum()) % 1000003, fwd_queries=0.0, mse=0.0, ms=0.0), 0

    def icp_align(self, s, t, out, params):
        return self._align_out(s, t, out)

    def icp_align_rejected(self, s, t, out, params, chain, return_trace=False):
        return self._align_out(s, t, out) + ([],)

    def icp_align_gicp(self, s, t, out, params, chain=(), return_trace=False):
        return self._align_out(s, t, out) + ([],)

    def fpfh(self, s, radius, return_counts=False, **kw):
        f = np.zeros((self.size(s), 33), F32)
        return (f, np.zeros(self.size(s), np.uint32)) if return_counts else f

    def boundary(self, s, radius, return_gap=False, return_counts=False, **kw):
        return np.zeros(self.size(s), bool), np.zeros(self.size(s), F32), np.zeros(self.size(s), np.uint32)

    def align_prerejective(self, s, t, sf, tf, **kw):
        return dict(converged=False, inliers=0, T=np.eye(4, dtype=F32))

    def pose_scores(self, s, t, T, max_dist, fma=False):
        return np.zeros(len(T), np.uint32), np.full(len(T), np.finfo(F64).max)

    def fitness(self, s, t, T, **kw):
        p, _ = self._move(self._get(s).pts, None, T, F32)
        return float(self._nn(p, self._get(t).pts)[1].astype(F64).mean()) if len(p) and self.size(t) else np.finfo(F64).max

    def pair_moments2(self, s, t, max_dist, origin, **kw):
        q, m, d = self.correspondences(s, t, max_dist)
        row = np.zeros(32)
        row[0], row[1:4], row[31] = len(q), origin, float(d.astype(F64).sum())
        return row

    def pair_moments2_batch(self, pairs, max_dist, origin, **kw):
        return [self.pair_moments2(s, t, max_dist, origin) for s, t in pairs]

    def ring_step(self, posed, raw, edges, poses, max_dist, origin, **kw):
        for d, s, T in zip(posed, raw, poses):
            self.transform(d, s, T)
        return np.asarray(poses, F64), dict(rows=np.zeros((len(edges), 32)), timing_ms=(0.0, 0.0, 0.0), pair_n=[0.0] * len(edges), lum_iterations=1,
                                            lum_pose=np.zeros((len(poses), 6)), pair_T=np.zeros((len(edges), 4, 4), F32), pair_mse=[0.0] * len(edges))

    def seq_run(self, raw, target, source, out, params, poses, repeat=1):
        self.transform(target, raw[0], poses[0])
        for v in range(1, len(raw)):
            self.transform(source, raw[v], poses[v])
            self.icp_align(source, target, out, params)
            self.append(target, out)
        return np.asarray(poses, F64), []


# ------------------------------------------------------------------ scenarios

PROLOGUE = [("upload", dict(slot=8, cloud="q:257")), ("upload", dict(slot=9, cloud="q:700"))]      # the two query slots

KINDS = {1: "ordering + sorted copy + boxes", 2: "set grid + pose + gsorted", 3: "model grid", 4: "align seeds", 5: "fused-batch pair records",
         6: "normals"}
S, R, T_, X, Y = 0, 1, 2, 3, 4          # the slot under test, its raw scan, a target, two spare slots


def state_on(s=S, r=R, t=T_, n=3000, nt=3000):
    """every kind of cached state on slot s: a raw scan posed by transform (a known pose of its set), aligned twice against t
    (ordering, sorted copy and boxes of both; the source grid of the reverse search and its gsorted; the seeds of the second
    align), searched by knn (model grid), given normals, and paired in a fused batch"""
    return [("upload", dict(slot=r, cloud="r1:%d" % n)), ("upload", dict(slot=t, cloud="v0:%d" % nt)),
            ("transform", dict(dst=s, src=r, pose="prior1")),
            ("icp_align", dict(src=s, tgt=t, out=-1, max_iter=1, max_dist=4.0)),
            ("icp_align", dict(src=s, tgt=t, out=-1, max_iter=1, max_dist=4.0)),
            ("knn", dict(src=8, tgt=s, k=9)),
            ("estimate_normals", dict(slots=[s, t], k=8)),
            ("correspondences", dict(src=s, tgt=t, reciprocal=True)), ("pair_moments2", dict(src=t, tgt=s)),
            ("pose_scores", dict(src=s, tgt=t)), ("fitness", dict(src=t, tgt=s, pose="nudge")),
            ("fpfh", dict(slot=s, radius=round(3.0 * spacing(n), 3))), ("boundary", dict(slot=s, radius=round(3.0 * spacing(n), 3))),
            ("pair_moments2_batch", dict(pairs=[[s, t], [t, s]]))]


# the mutator applied with the slot under test as DESTINATION, and (where it has a distinct source) as SOURCE
def tails(n=3000, nt=3000):
    h, small = spacing(n), min(n, nt, 1025)
    as_dst = {
        "upload": [("upload", dict(slot=S, cloud="v2:%d" % small))],
        "clear": [("clear", dict(slot=S))],
        "reserve": [("reserve", dict(slot=S, cap=7000))],
        "copy": [("copy", dict(dst=S, src=T_))],
        "append": [("nn", dict(src=8, tgt=T_)), ("append", dict(dst=S, src=T_))],
        "set_global_base": [("set_global_base", dict(slot=S, base=5000))],
        "append_range": [("append_range", dict(dst=S, src=T_, begin=nt // 30, count=nt // 4, base=40000))],
        "transform": [("transform", dict(dst=S, src=S, pose="nudge"))],
        "transform_f32": [("transform_f32", dict(dst=S, src=S, pose="nudge"))],
        "transform_batch": [("transform_batch", dict(dst=[S, X], src=[S, T_], pose=["nudge", "turn"]))],
        "upload_normals": [("upload_normals", dict(slot=S))],
        "estimate_normals": [("estimate_normals", dict(slots=[S], k=20))],
        "denoise": [("denoise", dict(slot=S, threshold=4, length=round(2.5 * h, 3)))],
        "voxel_grid": [("voxel_grid", dict(dst=S, src=S, leaf=round(2 * h, 3)))],
        "statistical_outlier_removal": [("statistical_outlier_removal", dict(dst=S, src=S, mean_k=8, mul=1.0))],
        "radius_outlier_removal": [("radius_outlier_removal", dict(dst=S, src=S, radius=round(1.5 * h, 3), min_neighbors=4))],
        "extract_indices": [("extract_indices", dict(dst=S, src=S, stride=3, negative=False))],
        "segment_plane": [("segment_plane", dict(dst=S, src=S, threshold=round(0.5 * h, 3), seed=1, negative=True))],
        "mls": [("mls", dict(dst=S, src=S, radius=round(3 * h, 3), compute_normals=False))],
        "iss_keypoints": [("iss_keypoints", dict(dst=S, src=S, salient=round(4 * h, 3), non_max=round(3 * h, 3)))],
        "icp_align": [("icp_align", dict(src=S, tgt=T_, out=S, max_iter=3, max_dist=4.0))],
        "icp_align_rejected": [("icp_align_rejected", dict(src=S, tgt=T_, out=S, max_iter=3, max_dist=4.0))],
        "icp_align_gicp": [("icp_align_gicp", dict(src=S, tgt=T_, out=S, max_iter=2, max_dist=4.0))],
        "ring_step": [("upload", dict(slot=X, cloud="v2:%d" % small)), ("upload", dict(slot=Y, cloud="v1:%d" % small)),
                      ("ring_step", dict(posed=[S, 5], raw=[X, Y], pose=["nudge", "eye"], max_dist=6.0))],
        "seq_run": [("upload", dict(slot=X, cloud="r0:%d" % small)), ("upload", dict(slot=Y, cloud="r1:%d" % small)),
                    ("seq_run", dict(raw=[X, Y], target=S, source=5, out=6, pose=["prior0", "prior1"], max_dist=6.0))],
    }
    as_src = {
        "copy": [("copy", dict(dst=X, src=S))],
        "append": [("append", dict(dst=X, src=S))],
        "append_range": [("append_range", dict(dst=X, src=S, begin=n // 12, count=n // 3, base=777))],
        "transform": [("transform", dict(dst=X, src=S, pose="nudge"))],
        "transform_f32": [("transform_f32", dict(dst=X, src=S, pose="turn"))],
        "transform_batch": [("transform_batch", dict(dst=[X, T_], src=[S, T_], pose=["nudge", "back"]))],
        "voxel_grid": [("voxel_grid", dict(dst=FILTER_DST, src=S, leaf=round(2 * h, 3)))],
        "statistical_outlier_removal": [("statistical_outlier_removal", dict(dst=FILTER_DST, src=S, mean_k=8, mul=1.0))],
        "radius_outlier_removal": [("radius_outlier_removal", dict(dst=X, src=S, radius=round(1.5 * h, 3), min_neighbors=4))],
        "extract_indices": [("extract_indices", dict(dst=X, src=S, stride=2, negative=True))],
        "segment_plane": [("segment_plane", dict(dst=FILTER_DST, src=S, threshold=round(0.5 * h, 3), seed=2, negative=False))],
        "mls": [("mls", dict(dst=X, src=S, radius=round(3 * h, 3), compute_normals=True))],
        "iss_keypoints": [("iss_keypoints", dict(dst=FILTER_DST, src=S, salient=round(4 * h, 3), non_max=round(3 * h, 3)))],
        "icp_align": [("icp_align", dict(src=S, tgt=T_, out=X, max_iter=3, max_dist=4.0))],
        "icp_align_rejected": [("icp_align_rejected", dict(src=S, tgt=T_, out=X, max_iter=1, max_dist=4.0))],
        "icp_align_gicp": [("icp_align_gicp", dict(src=S, tgt=T_, out=X, max_iter=2, max_dist=4.0))],
        "align_prerejective": [("align_prerejective", dict(src=S, tgt=T_, radius=round(5 * h, 3), seed=3))],
        "ring_step": [("upload", dict(slot=Y, cloud="v2:%d" % small)), ("ring_step", dict(posed=[X, 5], raw=[R, Y], pose=["prior1", "eye"], max_dist=6.0))],
        "seq_run": [("upload", dict(slot=Y, cloud="r0:%d" % small)), ("seq_run", dict(raw=[Y, R], target=X, source=5, out=6, pose=["prior0", "prior1"], max_dist=6.0))],
    }
    return as_dst, as_src


# ring_step and seq_run read RAW scans: plain slots without normals, which the slot under test is not once it has normals and
# a pose -- as their source they get its raw scan R, whose ordering the posed copy shares (kinds 1 and 2 are the SET's)

# (kind, mutator, role) that no scenario can build, each with its reason; nothing else may be missing
INAPPLICABLE = {}
for _k in KINDS:
    INAPPLICABLE[(_k, "align_prerejective", "dst")] = "the entry has no output slot: it moves the source on the context's scratch clouds only"
for _k in (3, 4, 5, 6):
    for _m in ("ring_step", "seq_run"):
        INAPPLICABLE[(_k, _m, "src")] = ("the drivers read raw scans -- plain slots without normals, never searched themselves; the state of kinds 3 to 6 "
                                         "lives on the posed copy, and a raw slot only carries its set's ordering and grid (kinds 1 and 2)")


def shard_scenario(align):
    """a slot that was a shard (set_global_base / append_range), then the OUTPUT of an align"""
    a = dict(src=S, tgt=T_, out=X, max_iter=3, max_dist=4.0)
    pre = [("upload", dict(slot=S, cloud="v1:3000")), ("upload", dict(slot=T_, cloud="v0:3000")),
           ("upload", dict(slot=X, cloud="v2:700")), ("set_global_base", dict(slot=X, base=5000)),
           ("append_range", dict(dst=X, src=T_, begin=100, count=257, base=99000))]
    if align == "icp_align_gicp":
        pre.append(("estimate_normals", dict(slots=[S, T_], k=20)))
    return pre + [(align, a), ("append", dict(dst=X, src=T_)), ("nn", dict(src=8, tgt=X)),
                  # ... and a shard as the SOURCE: the output takes its table, to another slot and in place
                  ("set_global_base", dict(slot=S, base=123456)), (align, dict(a, out=Y)), (align, dict(a, out=S))]


def matrix_scenarios(n=3000, nt=3000):
    """'dst-<mutator>' / 'src-<mutator>': every kind of state on the slot under test, then the mutator with that slot as its
    destination / its source.  n, nt: sizes of the scan under test and of its target (the host test runs them smaller)"""
    as_dst, as_src = tails(n, nt)
    sc = {}
    # after the mutator a probe consumes what no search reads (seeds, winner table, pair records), the slot as source and as target
    for m, tail in as_dst.items():
        sc["dst-" + m] = PROLOGUE + state_on(n=n, nt=nt) + tail + [("probe", dict(slot=S, other=T_))]
    for m, tail in as_src.items():
        w = [x for x in OPS[m].writes(tail[-1][1]) if x not in (S, T_, FILTER_DST)][:1]
        sc["src-" + m] = PROLOGUE + state_on(n=n, nt=nt) + tail + [("probe", dict(slot=x, other=T_)) for x in w] + [("probe", dict(slot=S, other=T_))]
    return sc


def named_scenarios(n=3000):
    """every named scenario.  n: what the 3 000-point scans are run with (the host test, on the numpy context, takes fewer; the
    sizes that are the point of a scenario -- 1 025 + 700, 257, 65, 3, 0 -- stay)"""
    sc = matrix_scenarios(n, n)
    sc.update(_hand_written())
    if n != 3000:
        for name, seq in sc.items():
            sc[name] = [(op, dict(a, cloud=a["cloud"].replace(":3000", ":%d" % n)) if op == "upload" else a) for op, a in seq]
    return sc


def _hand_written():
    sc = {}
    # every align with out = another slot, out == src, out = -1, out = a slot that was a shard
    for al in ALIGNS:
        sc["shard-" + al] = PROLOGUE + shard_scenario(al)
        sc["out-none-" + al] = PROLOGUE + state_on() + [(al, dict(src=S, tgt=T_, out=-1, max_iter=3, max_dist=4.0)),
                                                        (al, dict(src=T_, tgt=S, out=-1, max_iter=1, max_dist=4.0))]
    # mvr_cloud_append's extended ordering, an old size that is no multiple of the 256-point tile: the partly filled last tile
    # (the slot is reserved BEFORE its first search: the ordering's buffers are sized by the capacity it is built at)
    sc["extend-1025+700"] = PROLOGUE + [("reserve", dict(slot=S, cap=4000)), ("upload", dict(slot=S, cloud="v0:1025")), ("upload", dict(slot=X, cloud="v1:700")),
                                        ("nn", dict(src=8, tgt=S)), ("nn", dict(src=8, tgt=X)), ("append", dict(dst=S, src=X)),
                                        ("upload", dict(slot=Y, cloud="v2:257")), ("nn", dict(src=Y, tgt=S)), ("append", dict(dst=S, src=Y))]
    # an append that cannot extend: the ordering is shared with a copy, which must go on answering for the old points
    sc["append-shared-ordering"] = PROLOGUE + [("reserve", dict(slot=S, cap=4000)), ("upload", dict(slot=S, cloud="v0:1025")), ("upload", dict(slot=X, cloud="v1:700")),
                                               ("nn", dict(src=8, tgt=S)), ("nn", dict(src=8, tgt=X)), ("copy", dict(dst=Y, src=S)), ("nn", dict(src=8, tgt=Y)),
                                               ("append", dict(dst=S, src=X)), ("nn", dict(src=8, tgt=Y))]
    # the append pairs: self-append, into an empty slot, with / without normals on either side
    sc["append-pairs"] = PROLOGUE + [("upload", dict(slot=S, cloud="v0:700")), ("upload", dict(slot=X, cloud="v1:257")), ("upload_normals", dict(slot=X)),
                                     ("append", dict(dst=Y, src=X)), ("append", dict(dst=Y, src=Y)), ("append", dict(dst=Y, src=S)),
                                     ("append", dict(dst=S, src=X)), ("upload_normals", dict(slot=S)), ("append", dict(dst=S, src=X)),
                                     ("append", dict(dst=S, src=5)), ("append", dict(dst=5, src=5))]
    # a slot shrunk by a filter, then searched and aligned against
    sc["shrunk-by-a-filter"] = PROLOGUE + state_on() + [("extract_indices", dict(dst=T_, src=T_, stride=3, negative=False)), ("nn", dict(src=S, tgt=T_)),
                                                        ("icp_align", dict(src=S, tgt=T_, out=X, max_iter=3, max_dist=4.0)),
                                                        ("radius_outlier_removal", dict(dst=T_, src=T_, radius=round(1.5 * spacing(1000), 3), min_neighbors=4)),
                                                        ("icp_align_rejected", dict(src=S, tgt=T_, out=-1, max_iter=1, max_dist=4.0))]
    # a target that shrinks between two aligns of the same source: seed positions beyond the new size
    sc["target-shrinks-between-aligns"] = PROLOGUE + [("upload", dict(slot=S, cloud="v1:3000")), ("upload", dict(slot=T_, cloud="v0:3000")),
                                                      ("icp_align", dict(src=S, tgt=T_, out=-1, max_iter=1, max_dist=4.0)),
                                                      ("upload", dict(slot=T_, cloud="v0:257")),
                                                      ("icp_align", dict(src=S, tgt=T_, out=-1, max_iter=1, max_dist=4.0)),
                                                      ("upload", dict(slot=T_, cloud="v0:3000")), ("icp_align", dict(src=S, tgt=T_, out=X, max_iter=1, max_dist=4.0)),
                                                      ("extract_indices", dict(dst=T_, src=T_, stride=7, negative=False)),
                                                      ("icp_align", dict(src=S, tgt=T_, out=X, max_iter=1, max_dist=4.0))]
    # posed scans through the ring pass, twice (the second pass is seeded), then one posed slot changed in place between passes
    ring = dict(posed=[S, X, Y], raw=[R, T_, 5], pose=["prior0", "prior1", "prior2"], max_dist=6.0)
    sc["posed-scan-ring"] = PROLOGUE + [("upload", dict(slot=R, cloud="r0:3000")), ("upload", dict(slot=T_, cloud="r1:3000")), ("upload", dict(slot=5, cloud="r2:1025")),
                                        ("ring_step", ring), ("ring_step", ring), ("icp_align", dict(src=X, tgt=S, out=X, max_iter=1, max_dist=4.0)),
                                        ("pair_moments2_batch", dict(pairs=[[S, X], [X, Y], [Y, S]])), ("transform", dict(dst=Y, src=Y, pose="nudge")),
                                        ("ring_step", ring)]
    # a posed scan aligned against the growing model, as the sequential mode does by hand
    sc["posed-scan-align"] = PROLOGUE + [("upload", dict(slot=R, cloud="r0:3000")), ("upload", dict(slot=5, cloud="r1:3000")), ("transform", dict(dst=T_, src=R, pose="prior0")),
                                         ("reserve", dict(slot=T_, cap=8000)), ("transform", dict(dst=S, src=5, pose="prior1")),
                                         ("icp_align", dict(src=S, tgt=T_, out=X, max_iter=1, max_dist=4.0)), ("append", dict(dst=T_, src=X)),
                                         ("transform", dict(dst=S, src=5, pose="prior1")), ("icp_align", dict(src=S, tgt=T_, out=X, max_iter=3, max_dist=4.0))]
    # upload in every size relation, n = 0 and n = 3, on a slot with state
    sc["upload-sizes"] = PROLOGUE + state_on(n=1025, nt=700) + [("upload", dict(slot=S, cloud="v2:3000")), ("nn", dict(src=8, tgt=S)), ("upload", dict(slot=S, cloud="v0:3000")),
                                                                ("nn", dict(src=8, tgt=S)), ("upload", dict(slot=S, cloud="v1:257")), ("upload", dict(slot=S, cloud="empty")),
                                                                ("upload", dict(slot=S, cloud="v1:3")), ("upload", dict(slot=T_, cloud="v0:3")),
                                                                ("icp_align", dict(src=S, tgt=T_, out=X, max_iter=1, max_dist=400.0)), ("upload", dict(slot=S, cloud="v1:65"))]
    # non-finite points, with the entries whose own tests admit them: k-NN and the radius filter
    sc["non-finite"] = PROLOGUE + [("upload", dict(slot=S, cloud="v0:700")), ("knn", dict(src=8, tgt=S, k=9)), ("upload", dict(slot=S, cloud="dirty:700")),
                                   ("knn", dict(src=8, tgt=S, k=17)), ("copy", dict(dst=X, src=S)), ("append", dict(dst=X, src=S)), ("clear", dict(slot=S))]
    return sc


POSED_SCAN = ("posed-scan-ring", "posed-scan-align")          # the grid kernels must have run in these (culled mode)


# ---- what a sequence covers: (kind of state, mutator, role of the slot that carried it)

def _built(name, a, posed):
    """kinds of state the call builds: {slot: kinds}"""
    out = {}

    def add(s, *k):
        out.setdefault(s, set()).update(k)
    if name in ("nn", "correspondences", "pair_moments2", "fitness"):
        add(a["src"], 1); add(a["tgt"], 1)
    if name in ALIGNS:
        add(a["src"], 1, 4); add(a["tgt"], 1, 4)
        if posed.get(a["src"]):
            add(a["src"], 2)
    if name in ("knn", "pose_scores"):
        add(a["tgt"], 3)
    if name in ("fpfh", "boundary"):
        add(a["slot"], 3)
    if name == "upload_normals":
        add(a["slot"], 6)
    if name == "estimate_normals":
        for s in a["slots"]:
            add(s, 3, 6)
    if name == "pair_moments2_batch":
        for pair in a["pairs"]:
            for x in pair:
                add(x, 1, 5)
                if posed.get(x):
                    add(x, 2)
    if name == "ring_step":
        for s in a["posed"]:
            add(s, 1, 2, 5)
    return out


ORDER_SENSITIVE = ("pair_moments2", "pair_moments2_batch", "ring_step", "seq_run", "fitness", "align_prerejective") + ALIGNS      # return f64 sums taken in the order of a slot's ordering
CONSUMERS = ("probe", "pair_moments2_batch", "ring_step") + ALIGNS


def _sources(name, a):
    if name in ("ring_step", "seq_run"):
        return list(a["raw"])
    if name == "transform_batch":
        return list(a["src"])
    return [a["src"]] if "src" in a else []


def _posed_pairs(name, a):
    if name == "transform":
        return [(a["dst"], a["src"])]
    if name == "transform_batch":
        return list(zip(a["dst"], a["src"]))
    if name == "ring_step":
        return list(zip(a["posed"], a["raw"]))
    return []


def coverage(seq):
    """the (kind, mutator, role) cells a sequence exercises: the mutator is applied while the slot in that role carries
    state of that kind (built since the last call that rewrote the slot's points).  A raw scan carries kinds 1 and 2 of the
    posed copy made from it: the ordering and the grid are the point SET's."""
    st, posed, share, cells, pending = {}, {}, {}, set(), []
    for name, a in seq:
        op = OPS[name]
        dsts = list(op.writes(a)) if op.kind == "mutator" else []
        if name in CONSUMERS:               # seeds and pair records are read by aligns and batches only: a cell of theirs counts once one follows
            cells |= {c for c, slots in pending if slots & set(op.reads(a))}
            pending = [(c, slots) for c, slots in pending if not slots & set(op.reads(a))]
        if op.kind == "mutator":
            found = set()
            for s in dsts:
                found |= {((k, name, "dst"), s) for k in st.get(s, ())}
            for s in _sources(name, a):
                if s not in dsts:
                    found |= {((k, name, "src"), s) for k in st.get(s, ())}
            cells |= {c for c, s in found if c[0] not in (4, 5)}
            pending += [(c, {s} | set(dsts)) for c, s in found if c[0] in (4, 5)]
            if name not in POINT_PRESERVING:
                for s in dsts:
                    st[s], posed[s] = set(), False
                    share = {d: r for d, r in share.items() if d != s and r != s}
            for d, s in _posed_pairs(name, a):
                if d != s:
                    posed[d], share[d] = True, s
        for s, ks in _built(name, a, posed).items():
            if s not in dsts or name in POINT_PRESERVING + ("ring_step",):
                st.setdefault(s, set()).update(ks)
        for d, s in share.items():
            st.setdefault(s, set()).update(st.get(d, set()) & {1, 2})
    return cells


def required_cells():
    need = set()
    for name in MUTATORS:
        op = OPS[name]
        for k in KINDS:
            need.add((k, name, "dst"))
            if op.src_role:
                need.add((k, name, "src"))
    return need


# ---- seeded random sequences (Checker.run_random draws them)

SEEDS = tuple(range(101, 111))
RANDOM_STEPS = 30
RANDOM_PROLOGUE = PROLOGUE + [("upload", dict(slot=0, cloud="v1:3000")), ("upload", dict(slot=1, cloud="v0:3000")), ("upload", dict(slot=2, cloud="v2:1025"))]
