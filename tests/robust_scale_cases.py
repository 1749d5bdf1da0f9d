"""Crafted inputs for the exact-median robust scale (K7: bpvo_amd/csrc/gn_median.h, bracket_chunk in gn_common.h).

Residuals are I_cur(warp) - I_ref(point) and the current image is free, so crafted IMAGES give crafted residual multisets through the
existing C ABI: ties, bulk zeros, two-valued keys, a handful of valid points.  Every case names the property it is built for;
`check_property` computes that property from residuals and valid flags (the oracle's in tests/test_robust_scale_inputs_cpu.py, so that
tests/test_gpu_robust_scale.py cannot silently test nothing).

This module also holds the plain numpy restatement of the scale rule (`keys_of`, `plain_median`, `plain_scale`, `ScaleTracker`) and a
numpy mirror of the selection's path decisions (`PathModel`: bracketed or full, where the candidates live, how the selection finishes),
which predicts the differences of bpvo_hip_median_path_counts.  Nothing here reads the GPU library.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np

from bpvo_amd import synth
from util import make_params

# ---- the constants of gn_median.h the properties depend on (kept in step by hand: MED_THREADS / MED_COPIES / MED_CACHE and their _B forms,
# MED_BINS, K6_BLOCK; MED_REL_FLOOR / MED_REL_GAIN and the first-use width of the bracket rule at the end of median_block)
MED_BINS = 2048
CHUNK = 256                                            # points per bracket chunk (K6_BLOCK): one candidate segment per chunk
SHAPES = {1024: dict(NT=1024, COPIES=4, CACHE=20480),  # median_finish_kernel, launches of up to 256 workspaces
          512: dict(NT=512, COPIES=2, CACHE=7168)}     # launches of more than 256 workspaces; the persistent and team kernels run 512 threads too
REL_FIRST, REL_FLOOR, REL_GAIN, REL_MAX = np.float32(0.25), np.float32(0.01), np.float32(2.0), np.float32(0.5)
TOL = np.float32(1e-6)                                 # the freeze rule: recompute while |delta sigma| > 1e-6


def lds_room(shape):
    """Most candidates the bracketed path gathers into LDS: CACHE - 2 NT words (18432 / 6144)."""
    s = SHAPES[shape]
    return s["CACHE"] - 2 * s["NT"]


def tx_pose(tx):
    T = np.eye(4, dtype=np.float32)
    T[0, 3] = tx
    return T


IDENTITY = np.eye(4, dtype=np.float32)


# ---- the plain reference of the scale rule ---------------------------------------------------------------------------------------------------
def keys_of(r, valid, C):
    """|r| of the valid entries in channel-major order (replicateValidFlags + the copy loop of estimateScale): f32 [n]."""
    r = np.asarray(r, np.float32).reshape(C, -1)
    return np.abs(r[:, np.asarray(valid).reshape(-1) != 0]).reshape(-1)


def order_statistics(a):
    """(x[n/2 - 1], x[n/2]) of a (n >= 2), by np.partition."""
    n = a.size
    part = np.partition(a, [n // 2 - 1, n // 2])
    return np.float32(part[n // 2 - 1]), np.float32(part[n // 2])


def plain_median(a):
    """median() of bpvo/utils.h:224-252: empty -> 0, n < 3 -> first entry, odd -> middle, even -> f32(f64(f32(lo + hi)) / 2)."""
    n = a.size
    if n == 0:
        return np.float32(0.0)
    if n < 3:
        return np.float32(a[0])
    lo, hi = order_statistics(a)
    if n % 2:
        return hi
    return np.float32(np.float64(np.float32(lo + hi)) / 2.0)


def plain_scale(a):
    """(1.4826f * (1 + 5 / f32(n - 6 as uint64))) * median, < 1e-6 -> 1 (bpvo/mestimator.cc:452-490).  n - 6 wraps for n < 6 (to 2^64 - k,
    which rounds to 2^64 in f32 as in f64) and is 0 for n = 6: the factor is then infinite."""
    n = a.size
    nm6 = np.float32(float((n - 6) % (1 << 64)))
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.float32(np.float32(1.4826) * np.float32(np.float32(1.0) + np.float32(5.0) / nm6)) * plain_median(a)
    s = np.float32(s)
    if np.float64(s) < 1e-6:
        s = np.float32(1.0)
    return s


class ScaleTracker:
    """AutoScaleEstimator: scale 1 after reset, recomputed while the last change exceeded 1e-6 (a NaN change freezes it too)."""

    def __init__(self):
        self.scale, self.delta = np.float32(1.0), np.float32(1e10)

    def step(self, a):
        """-> (sigma, recomputed)"""
        if not (self.delta > TOL):
            return self.scale, False
        s = plain_scale(a)
        with np.errstate(invalid="ignore"):
            self.delta = np.float32(abs(np.float32(s - self.scale)))
        self.scale = s
        return s, True


def bits(x):
    return int(np.float32(x).view(np.uint32))


def first_use_bracket(median):
    """[lo_key, hi_key) after the first selection of a level: +-25 % of the median, in f32."""
    m = np.float32(median)
    return bits(m * np.float32(np.float32(1.0) - REL_FIRST)), bits(m * np.float32(np.float32(1.0) + REL_FIRST)) + 1


class PathModel:
    """The path decisions of median_block for one workspace, from the keys of every linearisation at which the estimator recomputes."""

    def __init__(self):
        self.valid, self.last, self.lo, self.hi = False, np.float32(0.0), 0, 0

    def step(self, a, n_points=0):
        """a: keys_of(...) of a recomputing linearisation, n_points: the template's points (one candidate segment per CHUNK of them) ->
        dict(path, n, m, below, nbits, in_lds{shape}, bin: keys of the fullest selected first-digit bin, split)"""
        n = a.size
        k = a.view(np.uint32)
        out = dict(path="full", n=n)
        if self.valid:
            below, m = int((k < self.lo).sum()), int(((k >= self.lo) & (k < self.hi)).sum())
            k_hi = n // 2
            k_lo = k_hi - 1 if (n % 2 == 0 and n > 0) else k_hi
            rng = self.hi - self.lo
            out.update(m=m, below=below, range=rng)
            if n >= 3 and k_lo >= below and k_hi < below + m and rng > 0:
                nbits = rng.bit_length()
                d = np.sort(k[(k >= self.lo) & (k < self.hi)].astype(np.int64) - self.lo)
                sh = max(nbits - 11, 0)
                b_lo, b_hi = d[k_lo - below] >> sh, d[k_hi - below] >> sh
                fullest = max(int(((d >> sh) == b_lo).sum()), int(((d >> sh) == b_hi).sum()))
                out.update(path="bracketed", nbits=nbits, split=bool(b_lo != b_hi), bin=fullest,
                           in_lds={s: m <= lds_room(s) and -(-n_points // CHUNK) < (SHAPES[s]["COPIES"] - 1) * MED_BINS for s in SHAPES},
                           more_passes={s: nbits > 11 and fullest > SHAPES[s]["NT"] for s in SHAPES})
        if out["path"] == "full" and n >= 3:
            lo, hi = order_statistics(a)
            p_lo, p_hi = bits(lo) >> 20, bits(hi) >> 20
            shared = int((((k >> 20) == p_lo) | ((k >> 20) == p_hi)).sum())
            out.update(split=bool(p_lo != p_hi), shared=shared, rescan={s: shared > SHAPES[s]["CACHE"] for s in SHAPES})
        med = plain_median(a)
        if n >= 3 and med > 0:
            rel = REL_FIRST
            if self.last > 0:
                rel = np.float32(min(REL_MAX, max(REL_FLOOR, np.float32(np.float32(REL_GAIN * np.float32(abs(np.float32(med - self.last)))) / self.last) + REL_FLOOR)))
            self.last = med
            self.lo = bits(med * np.float32(np.float32(1.0) - rel))
            self.hi = bits(med * np.float32(np.float32(1.0) + rel)) + 1
            self.valid = True
            out["rel"] = float(rel)
        else:
            self.valid = False
        out["median"] = float(med)
        return out


def multiset(a):
    """What a reader wants to know of a key multiset: n, distinct keys, the largest tie and its key, the two middle order statistics."""
    if a.size == 0:
        return dict(n=0, distinct=0, tie=0, tie_key=None, v_lo=None, v_hi=None)
    u, c = np.unique(a, return_counts=True)
    v_lo, v_hi = (np.float32(a[0]), np.float32(a[0])) if a.size < 2 else order_statistics(a)
    return dict(n=int(a.size), distinct=int(u.size), tie=int(c.max()), tie_key=float(u[c.argmax()]), v_lo=float(v_lo), v_hi=float(v_hi))


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------------
@dataclass
class Run:
    """One level-0 linearisation sequence: the first call resets the estimator, the rest do not."""
    cur: np.ndarray
    poses: list
    note: str = ""
    curs: list = None              # a current image of its own for every linearisation (None entries: keep the one in place)


@dataclass
class Start:
    """One estimate of a case: the current image, the starting pose, and the key count the first level-0 linearisation must see (or None)."""
    label: str
    cur: np.ndarray
    T0: np.ndarray
    reach_n: int = None


@dataclass
class Case:
    name: str
    prop: str                      # the property the case is built for
    rows: int
    cols: int
    params: dict                   # make_params keywords (descriptor, loss, ...)
    imgA: np.ndarray
    disp: np.ndarray
    K: np.ndarray
    b: float
    runs: list
    formulation: int = 0
    levels: int = 2
    expect: dict = field(default_factory=dict)

    @property
    def C(self):
        return 8 if self.params["descriptor"] == "bitplanes" else 1

    def make_params(self, binding, **kw):
        return make_params(binding, levels=self.levels, **{**self.params, **kw})

    def starts(self):
        """The estimates the case is run as: [Start] — every run's first current image from its first pose; tiny-n: one start per valid count."""
        if self.name == "tiny-n":
            return [Start(f"n{n}", self.runs[0].cur, tx_pose(tx), n) for n, tx in TINY_TX.items()]
        return [Start(f"run{k}", r.cur, r.poses[0], None) for k, r in enumerate(self.runs)]

    def create(self, binding, n_frames=2, n_pairs=1, **kw):
        """A context with the template in slot 0 and the first run's current image in slot 1."""
        ctx = binding.create(self.K, self.b, self.rows, self.cols, self.make_params(binding, **kw), n_frames=n_frames, n_pairs=n_pairs)
        if self.formulation:
            ctx.set_warp_formulation(self.formulation)
        ctx.frame_set_data(0, self.imgA, self.disp)
        ctx.frame_set_template(0)
        ctx.frame_set_data(1, self.runs[0].cur, self.disp)
        return ctx


PAIR_INDEX = 3                     # synth.make_pair(rows, cols, 3): the pair every case starts from
# found by scanning x-translations of the 160 x 120 intensity pair on the oracle: valid points at level 0 -> tx (metres)
TINY_TX = {7: 10.1435, 6: 10.145, 5: 10.155, 3: 10.175, 2: 10.185, 1: 10.195}
# found by bisection on the oracle: the first STRADDLE_SPLIT pixels (row-major) of the current image are the inverted template image, the rest
# 128 -> exactly half of the 73472 keys are 0
STRADDLE_SPLIT = 1098


def _pair(rows, cols):
    return synth.make_pair(rows, cols, PAIR_INDEX)


def _const(rows, cols, v):
    return np.full((rows, cols), v, np.uint8)


@functools.lru_cache(maxsize=None)
def case(name):
    small = dict(rows=120, cols=160)
    if name in ("ties-large", "same-exponent-flood", "bracket-flood"):
        # 16 grey levels: steps of 16 between neighbouring plateaus keep the edge pixels salient; NMS off keeps all of them
        d = _pair(240, 320)
        q = ((d["imgA"] // 16) * 16 + 8).astype(np.uint8)
        shifts = [IDENTITY, tx_pose(0.5), tx_pose(1.0)]      # the valid set shrinks: n changes, sigma changes by more than 1e-6, the ties stay
        runs = {"ties-large": [Run(_const(240, 320, 100), shifts, "median 36 in a tie of ~17 k: LDS gather, bin > NT, further passes"),
                               Run(_const(240, 320, 128), shifts, "median 8 in a tie of ~32 k: global segment walk, pass-3 rescan")],
                "same-exponent-flood": [Run(_const(240, 320, 128), [IDENTITY, tx_pose(0.5)], "first selection of a level: full path; then a bracketed one")],
                "bracket-flood": [Run(_const(240, 320, 128), [IDENTITY, IDENTITY], "second linearisation at the same pose")]}[name]
        prop = {"ties-large": "the largest tie exceeds 1024 keys and holds the median",
                "same-exponent-flood": "more than 20480 valid keys share the median's bits [30:20]",
                "bracket-flood": "more than 18432 keys inside [0.75, 1.25) x median"}[name]
        return Case(name, prop, 240, 320, dict(descriptor="intensity", loss="huber", nonMaxSuppRadius=0), q, d["dispA"], d["K"], d["b"], runs)
    d = _pair(120, 160)
    bp = dict(descriptor="bitplanes", loss="tukey", sigmaBitPlanes=-1.0)
    inv = (255 - d["imgA"]).astype(np.uint8)
    if name == "two-valued":
        flat = _const(120, 160, 128)
        return Case(name, "at most 4 distinct keys, most of them 0, median exactly 0, sigma 1", params=bp, imgA=d["imgA"], disp=d["dispA"], K=d["K"], b=d["b"],
                    runs=[Run(flat, [IDENTITY, tx_pose(0.3)], "a constant image has all-zero bit-planes: |r| is the template's bit; sigma 1 = the reset value freezes at once"),
                          Run(inv, [IDENTITY, IDENTITY, tx_pose(0.3), tx_pose(0.6)], "sigma 1.48 first, so that the median-0 selections after it recompute twice",
                              curs=[None, flat, None, None])], **small)
    if name == "two-valued-straddle":
        cur = _const(120, 160, 128).reshape(-1)
        cur[:STRADDLE_SPLIT] = inv.reshape(-1)[:STRADDLE_SPLIT]
        cur = cur.reshape(120, 160)
        return Case(name, "n even, the two middle keys differ in their top 11 bits (0 and a fraction)", params=bp, imgA=d["imgA"], disp=d["dispA"], K=d["K"], b=d["b"],
                    runs=[Run(cur, [IDENTITY, IDENTITY], "half of the keys are 0"),
                          Run(inv, [IDENTITY, IDENTITY], "inverted template: nearly every key is (nearly) 1; 8 channels flood the bracket at 160 x 120")], **small)
    if name == "all-zero":
        return Case(name, "every key is 0", params=dict(descriptor="intensity", loss="huber"), imgA=d["imgA"], disp=d["dispA"], K=d["K"], b=d["b"], formulation=2,
                    runs=[Run(d["imgA"], [IDENTITY, IDENTITY], "the template frame as its own current frame, disparity-space warp"),
                          Run(d["imgB"], [IDENTITY, IDENTITY, IDENTITY, IDENTITY], "another frame first, so that the all-zero selections after it recompute twice",
                              curs=[None, d["imgA"], None, None])], **small)
    if name == "bracket-miss":
        two = _const(120, 160, 128)
        two[:, 80:] = 255
        return Case(name, "the median of linearisation k + 1 lies outside the bracket derived from linearisation k", params=dict(descriptor="intensity", loss="huber"),
                    imgA=d["imgA"], disp=d["dispA"], K=d["K"], b=d["b"],
                    runs=[Run(two, [tx_pose(-3.0), tx_pose(3.0), tx_pose(-3.0), tx_pose(3.0), IDENTITY], "points land on the 128 half or on the 255 half")], **small)
    if name == "tiny-n":
        t = {n: tx_pose(tx) for n, tx in TINY_TX.items()}
        return Case(name, "valid counts 1, 2, 3, 5, 6 and 7 are reached; sigma is inf at n = 6", params=dict(descriptor="intensity", loss="huber"),
                    imgA=d["imgA"], disp=d["dispA"], K=d["K"], b=d["b"],
                    runs=[Run(d["imgB"], [t[7], t[5], t[3], t[2], t[1], t[3]], "n - 6 wraps below 6; n < 3 takes the first entry"),
                          Run(d["imgB"], [t[6], t[6], t[7]], "n = 6 at a level's first (full) selection, and again: inf - inf is NaN, the scale freezes at inf"),
                          Run(d["imgB"], [t[7], t[6], t[5]], "n = 6 behind a bracket (which it misses), n = 5 inside one"),
                          Run(d["imgB"], [t[1], t[2], t[5]], "n < 3 first: no bracket is derived")], **small)
    raise KeyError(name)


CASES = ["ties-large", "two-valued", "two-valued-straddle", "all-zero", "same-exponent-flood", "bracket-flood", "bracket-miss", "tiny-n"]
# narrow-bracket (hi_key - lo_key < 2^11) is absent: see the docstring of tests/test_robust_scale_inputs_cpu.py


def walk(ctx, cs, want_weights=True):
    """Drive cs through its runs on a context made by cs.create: [[dict(sigma, num_valid, r, valid, w)]] per run and linearisation."""
    out = []
    for k, run in enumerate(cs.runs):
        ctx.frame_set_data(1, run.cur, cs.disp)
        steps = []
        for i, T in enumerate(run.poses):
            if run.curs and run.curs[i] is not None:
                ctx.frame_set_data(1, run.curs[i], cs.disp)
            a = ctx.linearize(0, 0, 1, 0, T, reset_scale=(i == 0))
            steps.append(dict(sigma=np.float32(a["sigma"]), num_valid=a["num_valid"], r=ctx.get_residuals(0), valid=ctx.get_valid(0),
                              w=ctx.get_weights(0) if want_weights else None))
        out.append(steps)
    return out


def analyse(cs, walked):
    """The plain scale and the path model along walked (walk's output): [[dict(keys, sigma, recomputed, path (None where frozen), multiset)]]."""
    out = []
    for steps in walked:
        tracker, model, rows = ScaleTracker(), PathModel(), []
        for s in steps:
            a = keys_of(s["r"], s["valid"], cs.C)
            sigma, rec = tracker.step(a)
            rows.append(dict(keys=a, sigma=sigma, recomputed=rec, path=model.step(a, np.asarray(s["valid"]).size) if rec else None, multiset=multiset(a)))
        out.append(rows)
    return out


def predicted_counts(analysis):
    """(bracketed, full) selections the runs of a case must add to bpvo_hip_median_path_counts."""
    paths = [r["path"]["path"] for rows in analysis for r in rows if r["recomputed"]]
    return paths.count("bracketed"), paths.count("full")


def check_property(cs, analysis):
    """Assert that the case has the property it is built for; returns a one-line description of what was reached."""
    A = analysis
    first = A[0][0]
    ms = first["multiset"]
    every = [r for rows in A for r in rows]
    rec = [r for r in every if r["recomputed"]]
    paths = [r["path"] for r in rec]
    if cs.name == "ties-large":
        for rows in A:
            for r in rows:
                m = r["multiset"]
                assert m["tie"] > 1024 and m["tie_key"] == m["v_lo"] == m["v_hi"], m
                assert m["distinct"] <= 16, m
            assert all(r["recomputed"] for r in rows), "n changes sigma by more than 1e-6 at every step"
        br = [p for p in paths if p["path"] == "bracketed"]
        assert len(br) == 4 and all(p["bin"] > 1024 and p["more_passes"][1024] and p["more_passes"][512] for p in br), br
        assert any(p["in_lds"][1024] for p in br) and any(not p["in_lds"][1024] for p in br), "both homes of the candidates"
    elif cs.name == "two-valued":
        assert ms["distinct"] <= 4, ms
        for r in A[0] + A[1][1:]:      # (translated poses interpolate along the image border: a few fractions join the two keys)
            m = r["multiset"]
            assert m["tie_key"] == 0.0 and 2 * m["tie"] > m["n"] and m["v_lo"] == m["v_hi"] == 0.0, m
            assert r["sigma"] == 1.0
        assert [r["recomputed"] for r in A[0]] == [True, False] and [r["recomputed"] for r in A[1]] == [True, True, True, False]
        assert all(p["path"] == "full" for p in paths) and len(paths) == 4      # a median of 0 derives no bracket: full again
        assert paths[0]["rescan"][1024], "38 k zeros share the median's top bits"
    elif cs.name == "two-valued-straddle":
        assert ms["n"] % 2 == 0 and ms["v_lo"] != ms["v_hi"] and bits(ms["v_lo"]) >> 20 != bits(ms["v_hi"]) >> 20, ms
        assert ms["v_lo"] == 0.0 and paths[0]["path"] == "full" and paths[0]["split"]
        flood = [p for p in paths if p["path"] == "bracketed"]
        assert flood and all(p["m"] > lds_room(1024) for p in flood), "the inverted run: a bracket of more keys than either shape gathers"
    elif cs.name == "all-zero":
        assert all(r["multiset"]["distinct"] == 1 and r["multiset"]["tie_key"] == 0.0 and r["sigma"] == 1.0 for r in A[0] + A[1][1:])
        assert [r["recomputed"] for r in A[0]] == [True, False] and [r["recomputed"] for r in A[1]] == [True, True, True, False]
        assert ms["n"] > 1024 and all(p["path"] == "full" for p in paths) and len(paths) == 4
    elif cs.name == "same-exponent-flood":
        assert paths[0]["path"] == "full" and paths[0]["shared"] > 20480 and paths[0]["rescan"][1024] and paths[0]["rescan"][512], paths[0]
        assert paths[1]["path"] == "bracketed", paths[1]
    elif cs.name == "bracket-flood":
        a, med = first["keys"], plain_median(first["keys"])
        lo, hi = first_use_bracket(med)
        inside = int(((a.view(np.uint32) >= lo) & (a.view(np.uint32) < hi)).sum())
        assert inside > lds_room(1024) > lds_room(512), inside
        p = paths[1]
        assert p["path"] == "bracketed" and p["m"] == inside and not p["in_lds"][1024] and not p["in_lds"][512], p
    elif cs.name == "bracket-miss":
        rows = A[0]
        assert all(r["recomputed"] for r in rows)
        model = PathModel()
        for k in range(len(rows) - 1):
            model.step(rows[k]["keys"])
            med = bits(plain_median(rows[k + 1]["keys"]))
            if k < 3:
                assert not (model.lo <= med < model.hi), (k, model.lo, med, model.hi)
                change = abs(rows[k + 1]["path"]["median"] / rows[k]["path"]["median"] - 1.0)
                assert change > 0.5, change
        assert [p["path"] for p in paths[:4]] == ["full"] * 4
    elif cs.name == "tiny-n":
        seen = {r["multiset"]["n"] for r in rec}
        assert {1, 2, 3, 5, 6, 7} <= seen, seen
        six = [r for r in rec if r["multiset"]["n"] == 6]
        assert six and all(np.isinf(r["sigma"]) for r in six)
        assert any(p["path"] == "bracketed" and p["n"] == 5 for p in paths), "a bracketed selection among a handful of keys"
        assert [r["recomputed"] for r in A[1]] == [True, True, False] and np.isinf(A[1][2]["sigma"]), "inf - inf is NaN: the scale freezes"
    else:
        raise KeyError(cs.name)
    b, f = predicted_counts(A)
    return (f"{cs.name}: n={ms['n']} distinct={ms['distinct']} largest tie={ms['tie']} at {ms['tie_key']:g}, middle keys {ms['v_lo']:g} / {ms['v_hi']:g}; "
            f"selections bracketed={b} full={f}")
