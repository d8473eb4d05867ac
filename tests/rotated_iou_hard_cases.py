"""Box pairs off the nuScenes-like range of rotated_nms_cases.py, for `rotated_iou_bev` and `rotated_nms_bev`: yaws many
turns from zero, barriers and strips with an aspect of thousands, quarter-turn and axis yaws, far centres, scaled scenes;
closed forms that do not use `iou64`; and pairs frozen from the arithmetic before the relative angle was kept exact.

A family is a seeded builder of P = 256 pairs (a[P, 5], b[P, 5]) in float32, compared PAIR-WISE (P frames of 1 x 1 boxes),
so that the float64 clip stays at a few thousand pairs per test.  Unless a family says otherwise, B is A "moved and turned
a little": the centre moved by N(0, a quarter of A's SHORT side) in x and y, the sizes within 5 % of A's, the yaw A's plus
the family's offset and a twist of either sign, log-uniform in 1e-7 ... 1e-2 (1e-3 for strips, where 1e-2 turns the ends
apart).  The stress of these families is the RELATIVE ANGLE: its error acts over the half length against the width.  The
move is scaled by the short side so that every family keeps most of its pairs overlapping.  Turns are added to the yaw in
float64 and the sum is rounded to float32 once: the float32 values are the inputs, and the definition is evaluated on them.

Every builder asserts, on the float64 values, that a stated share of its pairs has IoU > 0.05 and that its stress is
there (`|yaw_a - yaw_b| > 2 pi k - 1`, an aspect above 1000, ...): a family cannot pass by showing nothing.

Domain: |yaw| <= YAW_DOMAIN = 4096 rad (about 650 turns).  The operator corrects the rounding of yaw_a - yaw_b to first
order; beyond the domain the second-order term is no longer below the bar (csrc/rotated_iou_arith.h, step 2).
"""
import functools
import math

import numpy as np

from rotated_nms_cases import BAR, _clip_pairs, _ok, ragged5

P = 256
TWO_PI = 2 * math.pi
YAW_DOMAIN = 4096.0
TURNS = (1, 3, 10, 100, 650)
OVERLAP = 0.05


def iou64_pairs(a, b):
    """a, b [P, 5] (any float dtype) -> float64 [P]: the definition of rotated_nms_cases.iou64 for the pairs (a[p], b[p])"""
    a, b = np.asarray(a, np.float64).reshape(-1, 5), np.asarray(b, np.float64).reshape(-1, 5)
    out = np.zeros(a.shape[0])
    with np.errstate(all="ignore"):
        ra, rb = np.hypot(a[:, 2], a[:, 3]) / 2, np.hypot(b[:, 2], b[:, 3]) / 2
        near = _ok(a) & _ok(b) & ((a[:, 0] - b[:, 0]) ** 2 + (a[:, 1] - b[:, 1]) ** 2 <= (ra + rb) ** 2)
    i = np.nonzero(near)[0]
    inter = _clip_pairs(a[i], b[i])
    out[i] = inter / (a[i, 2] * a[i, 3] + b[i, 2] * b[i, 3] - inter)
    return out


def op_pairs(a, b, device="cpu"):
    """the operator on the pairs (a[p], b[p]), as P frames of one box each: float32 [P]"""
    from accvlab.draw_heatmap import rotated_iou_bev

    a, b = np.array(a, np.float32).reshape(-1, 1, 5), np.array(b, np.float32).reshape(-1, 1, 5)      # copies: the families are read-only
    n = [1] * len(a)
    out = rotated_iou_bev(ragged5(a, n, device), ragged5(b, n, device)).tensor
    assert tuple(out.shape) == (len(a), 1, 1)
    return out.reshape(-1).cpu().numpy()


# ----------------------------------------------------------------------------------------------------------- the draws
def near_pairs(rng, n, dx, dy, *, yaw=(-math.pi, math.pi), offset=0.0, turns_a=0, turns_b=0, twist=(1e-7, 1e-2), centre=(-50.0, 50.0),
               swap=False, scale=1.0):
    """n pairs: A of dx x dy (each side within 20 %), B = A moved and turned a little (module docstring).  `offset` is added
    to B's yaw before the twist, `turns_a` / `turns_b` whole turns after it; `swap` writes B's rectangle with its sides
    exchanged (the caller puts the quarter turn into `offset`); `scale` multiplies centres and sizes of both."""
    size = np.array([dx, dy])[None] * rng.uniform(0.8, 1.2, (n, 2))
    xy = rng.uniform(centre[0], centre[1], (n, 2))
    ya = rng.uniform(yaw[0], yaw[1], n)
    move = rng.normal(0.0, 0.25, (n, 2)) * size.min(1)[:, None]
    size_b = size * rng.uniform(0.95, 1.05, (n, 2))
    tw = np.exp(rng.uniform(math.log(twist[0]), math.log(twist[1]), n)) * rng.choice([-1.0, 1.0], n)
    yb = ya + offset + tw
    if swap:
        size_b = size_b[:, ::-1]
    a = np.concatenate([xy * scale, size * scale, (ya + TWO_PI * turns_a)[:, None]], 1).astype(np.float32)
    b = np.concatenate([(xy + move) * scale, size_b * scale, (yb + TWO_PI * turns_b)[:, None]], 1).astype(np.float32)
    return a, b


def _cat(*parts):
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def _yaw_gap(a, b):
    return np.abs(a[:, 4].astype(np.float64) - b[:, 4].astype(np.float64))


def _aspect(x):
    return (np.maximum(x[:, 2], x[:, 3]) / np.minimum(x[:, 2], x[:, 3])).astype(np.float64)


CAR, BARRIER, THIN = (4.5, 1.9), (12.0, 0.3), (50.0, 0.02)
STRIP_TWIST = (1e-7, 1e-3)


def _car(rng, **kw):
    a, b = near_pairs(rng, P, *CAR, **kw)
    return a, b, 0.95, True


def _turns(rng, box, ka, kb, **kw):
    a, b = near_pairs(rng, P, *box, turns_a=ka, turns_b=kb, **kw)
    stress = (_yaw_gap(a, b) > TWO_PI * abs(ka - kb) - 1).all() and max(np.abs(a[:, 4]).max(), np.abs(b[:, 4]).max()) > TWO_PI * max(abs(ka), abs(kb)) - 4
    return a, b, 0.95, stress


def _barrier(rng, ka, kb):
    a, b, _, stress = _turns(rng, BARRIER, ka, kb, twist=STRIP_TWIST)
    return a, b, 0.95, stress and (_aspect(a) > 25).all()


def _thin(rng, offset):
    """50 x 0.02 strips whose yaws are `offset` apart, both within +-2 pi"""
    lo = max(-TWO_PI, -TWO_PI - offset) + 2e-3
    a, b = near_pairs(rng, P, *THIN, yaw=(lo, lo + min(TWO_PI, 2 * TWO_PI - abs(offset)) - 4e-3), offset=offset, twist=STRIP_TWIST)
    stress = ((_aspect(a) > 1000).all() and (np.abs(_yaw_gap(a, b) - abs(offset)) < 2e-3).all()
              and max(np.abs(a[:, 4]).max(), np.abs(b[:, 4]).max()) <= TWO_PI)
    return a, b, 0.95, stress


def _strips(rng):
    """50 x 0.1 and 200 x 0.1 strips, yaws 0, pi and 2 pi apart"""
    parts = [near_pairs(rng, P // 8, length, 0.1, offset=off, twist=STRIP_TWIST) for length in (50.0, 200.0) for off in (0.0, math.pi, TWO_PI, -TWO_PI)]
    a, b = _cat(*parts)
    return a, b, 0.95, (_aspect(a) > 300).all() and (np.abs(_yaw_gap(a, b) - TWO_PI) < 2e-3).sum() >= P // 4


def _far(rng):
    """cars whose centres are 1e3, 1e4, 1e5 m out (the moved centre lands on the float32 lattice there: 7.8 mm at 1e5), and
    whole scenes scaled by 1e-3, 1e3, 1e4 and 1e6"""
    parts = [near_pairs(rng, P // 8, *CAR, centre=(r, r + 50.0)) for r in (1e3, -1e4, 1e5)] + [near_pairs(rng, P // 8, *CAR, centre=(-1e5 - 50.0, -1e5))]
    parts += [near_pairs(rng, P // 8, *CAR, scale=s) for s in (1e-3, 1e3, 1e4, 1e6)]
    a, b = _cat(*parts)
    return a, b, 0.95, (np.abs(a[:P // 2, :2]).max(1) >= 1e3).all() and a[P // 2:, 2].min() < 0.01 and a[P // 2:, 2].max() > 1e6


def _swapped(rng):
    """B is A's rectangle written as (dy, dx, yaw + pi / 2), moved and turned a little"""
    a, b = near_pairs(rng, P, *CAR, offset=math.pi / 2, swap=True)
    return a, b, 0.95, (np.abs(_yaw_gap(a, b) - math.pi / 2) < 0.011).all() and (np.abs(a[:, 2] / b[:, 3] - 1) < 0.06).all()


def _mixed(rng):
    """100 x 0.05 strips crossing at 1e-3 ... 0.3 rad, a small box inside a big one at any angle, a 50 x 0.1 strip over a car"""
    n = P // 4
    cross = near_pairs(rng, 2 * n, 100.0, 0.05, twist=(1e-3, 0.3))
    big, small = near_pairs(rng, n, 6.0, 4.0, twist=(1e-2, math.pi))
    small[:, 2:4] = (big[:, 2:4] * rng.uniform(0.3, 0.6, (n, 2))).astype(np.float32)
    car, strip = near_pairs(rng, n, *CAR, twist=(1e-2, math.pi))
    strip[:, 2:4] = np.float32([50.0, 0.1])
    a, b = _cat(cross, (small, big), (strip, car))
    return a, b, 0.35, (_aspect(a[:2 * n]) > 1000).all() and (_yaw_gap(a, b)[:2 * n] > 9e-4).all()


def _quarter(rng):
    """yaws k pi / 2 apart, k = -8 ... 8 (sixteen pairs each), plus a twist of 1e-6; for odd k B's sides are exchanged, so that
    the rectangles nearly coincide whatever k"""
    parts = []
    for k in range(-8, 9):
        parts.append(near_pairs(rng, P // 16, *CAR, offset=k * math.pi / 2, swap=k % 2 == 1, twist=(1e-6, 1.0000001e-6)))
    a, b = _cat(*parts)
    q = _yaw_gap(a, b) / (math.pi / 2)
    return a, b, 0.95, (np.abs(q - np.round(q)) * (math.pi / 2) < 3e-6).all() and len(np.unique(np.round(q))) == 9


AXIS_YAWS = np.float32([0.0, -0.0, 1e-40, -1e-40, math.pi, -math.pi, math.pi / 2, -math.pi / 2])


def _axis(rng):
    """every ordered pair of the axis yaws: 0, -0.0, a denormal of either sign, +-pi and +-pi / 2 as float32, four draws each"""
    n = len(AXIS_YAWS)
    a, b = near_pairs(rng, 4 * n * n, *CAR)
    i, j = np.divmod(np.arange(4 * n * n) // 4, n)
    a[:, 4], b[:, 4] = AXIS_YAWS[i], AXIS_YAWS[j]
    stress = np.isin(a[:, 4], AXIS_YAWS).all() and np.signbit(a[:, 4]).any() and (np.abs(b[:, 4]) == np.float32(1e-40)).any() and np.float32(1e-40) > 0
    return a, b, 0.95, stress


FAMILIES = {"car, yaws in +-pi": (_car, {})}
for _k in TURNS:
    FAMILIES[f"car, A {_k} turns ahead"] = (_turns, dict(box=CAR, ka=_k, kb=0))
    FAMILIES[f"car, B {_k} turns ahead"] = (_turns, dict(box=CAR, ka=0, kb=_k))
    FAMILIES[f"car, -{_k} turns against +{_k}"] = (_turns, dict(box=CAR, ka=-_k, kb=_k))
    FAMILIES[f"barrier 12 x 0.3, A {_k} turns ahead"] = (_barrier, dict(ka=_k, kb=0))
FAMILIES.update({
    "thin 50 x 0.02, yaws 2 pi apart": (_thin, dict(offset=-TWO_PI)),
    "thin 50 x 0.02, yaws pi apart": (_thin, dict(offset=math.pi)),
    "strips 50 x 0.1 and 200 x 0.1, yaws 0, pi, 2 pi apart": (_strips, {}),
    "far centres and scaled scenes": (_far, {}),
    "sides exchanged and a quarter turn": (_swapped, {}),
    "strips crossing, box inside box, strip over car": (_mixed, {}),
    "quarter-turn differences": (_quarter, {}),
    "axis yaws": (_axis, {}),
})
NAMES = tuple(FAMILIES)


@functools.lru_cache(maxsize=None)
def family(name):
    """(a, b, want): float32 [P, 5] twice and the float64 IoU [P] of the pairs.  Cached: treat as read-only."""
    build, kw = FAMILIES[name]
    a, b, share, stress = build(np.random.default_rng(NAMES.index(name) + 7000), **kw)
    assert a.dtype == np.float32 and b.dtype == np.float32 and a.shape == b.shape and a.shape[0] >= P
    assert stress, f"{name}: the stress the family is named for is not in its draws"
    assert max(np.abs(a[:, 4]).max(), np.abs(b[:, 4]).max()) <= YAW_DOMAIN, f"{name}: a yaw outside the promised domain"
    want = iou64_pairs(a, b)
    got = float((want > OVERLAP).mean())
    assert got >= share, f"{name}: only {got:.2f} of the pairs overlap with IoU > {OVERLAP}, {share} stated"
    for x in (a, b, want):
        x.setflags(write=False)
    return a, b, want


# ---------------------------------------------------------------------------------------------------------- closed forms
def crossing_strips(seed=1):
    """(a, b, iou): two strips of widths w1, w2 in 0.02 ... 0.5 about one centre, crossing at theta in 0.05 ... pi / 2, of length
    1.5 (w1 + w2) / sin theta: the parallelogram they share spans at most (w1 + w2) / sin theta along either, so no end is
    inside the other and the intersection is w1 w2 / |sin theta|.  theta is the difference of the float32 yaws."""
    rng = np.random.default_rng(seed)
    theta = np.concatenate([[0.05, math.pi / 2], rng.uniform(0.05, math.pi / 2, P - 2)])
    w = np.concatenate([[[0.02, 0.02], [0.5, 0.02]], np.exp(rng.uniform(math.log(0.02), math.log(0.5), (P - 2, 2)))])
    ya = rng.uniform(-math.pi, math.pi, P)
    xy = rng.uniform(-50.0, 50.0, (P, 2))
    length = 1.5 * (w[:, 0] + w[:, 1]) / np.sin(theta)
    a = np.concatenate([xy, length[:, None], w[:, :1], ya[:, None]], 1).astype(np.float32)
    b = np.concatenate([xy, length[:, None], w[:, 1:], (ya + theta * rng.choice([-1.0, 1.0], P))[:, None]], 1).astype(np.float32)
    A, B = a.astype(np.float64), b.astype(np.float64)
    sin = np.abs(np.sin(A[:, 4] - B[:, 4]))
    assert (np.minimum(A[:, 2], B[:, 2]) > 1.2 * (A[:, 3] + B[:, 3]) / sin).all(), "an end of a strip is inside the other"
    inter = A[:, 3] * B[:, 3] / sin
    return a, b, inter / (A[:, 2] * A[:, 3] + B[:, 2] * B[:, 3] - inter)


def box_inside_box(seed=2):
    """(a, b, iou): a small box whose circumscribed circle lies inside the big box, at any relative yaw: area_small / area_big"""
    rng = np.random.default_rng(seed)
    big = np.concatenate([rng.uniform(-50.0, 50.0, (P, 2)), rng.uniform(2.0, 12.0, (P, 2)), rng.uniform(-math.pi, math.pi, (P, 1))], 1)
    room = big[:, 2:4].min(1) / 2
    r = room * rng.uniform(0.3, 0.7, P)                      # the small box's circumscribed radius
    along = rng.uniform(0.2, 1.4, P)                         # the direction of its diagonal
    off = rng.uniform(-1.0, 1.0, (P, 2)) * ((room - r) * 0.7)[:, None]      # in the big box's frame: |off| < room - r
    c, s = np.cos(big[:, 4]), np.sin(big[:, 4])
    xy = big[:, :2] + np.stack([off[:, 0] * c - off[:, 1] * s, off[:, 0] * s + off[:, 1] * c], 1)
    small = np.concatenate([xy, (2 * r * np.cos(along))[:, None], (2 * r * np.sin(along))[:, None], rng.uniform(-math.pi, math.pi, (P, 1))], 1)
    a, b = small.astype(np.float32), big.astype(np.float32)
    A, B = a.astype(np.float64), b.astype(np.float64)
    assert (np.hypot(A[:, 0] - B[:, 0], A[:, 1] - B[:, 1]) + np.hypot(A[:, 2], A[:, 3]) / 2 < B[:, 2:4].min(1) / 2).all()
    return a, b, A[:, 2] * A[:, 3] / (B[:, 2] * B[:, 3])


def rewritten_rectangles(seed=3):
    """(r, q, third): cars, pedestrians, trucks and barriers, the same rectangles written as (dy, dx, yaw + pi / 2), and a
    third box near each.  yaw + pi / 2 is rounded to float32: the two are 1.2e-7 rad apart at most in +-pi, 1e-6 of IoU."""
    rng = np.random.default_rng(seed)
    parts = [near_pairs(rng, P // 4, dx, dy, twist=(1e-2, 1.0)) for dx, dy in (CAR, (0.7, 0.7), (10.0, 2.8), BARRIER)]
    r, third = _cat(*parts)
    q = r.copy()
    q[:, 2], q[:, 3] = r[:, 3], r[:, 2]
    q[:, 4] = (r[:, 4].astype(np.float64) + math.pi / 2).astype(np.float32)
    return r, q, third


# ------------------------------------------------------------------------------------- what the bar does not cover
# The centre offset t = c_A - c_B is rotated into B's frame with float32 products: cy = ty * cB - tx * sB.  Each product is
# rounded by 2^-24 relative, cB and sB carry up to two ulp (2^-23) of the platform's cosf / sinf, tx and ty 2^-24: with
# |ty cB| + |tx sB| <= sqrt 2 |t| the across coordinate is off by up to sqrt 2 |t| 2^-22 = 3.4e-7 |t|, and two strips of width
# w that nearly coincide lose 2 / w of IoU per unit of it.  The families above move B by a quarter of the SHORT side, so the
# term is far below the bar; a strip moved metres ALONG its length has |t| / w in the hundreds, and there the operator is held
# to BAR + SHIFT_TERM |t| / w, not to the bar alone (measured: DESIGN 9o).
SHIFT_TERM = 2 * math.sqrt(2) * 2.0 ** -22          # 6.7e-7 per unit of |t| / w


def shifted_strips(seed=4):
    """(a, b, want, bound): 50 x 0.02 and 200 x 0.1 strips, B moved as in the families and then along A's length by N(0, a tenth of
    it); bound[p] = BAR + SHIFT_TERM |t| / w, |t| the centre distance and w the smallest of the pair's four sides"""
    rng = np.random.default_rng(seed)
    parts = []
    for dx, dy in (THIN, (200.0, 0.1)):
        a, b = near_pairs(rng, P // 2, dx, dy, twist=STRIP_TWIST)
        t = rng.normal(0.0, 0.1 * dx, P // 2)
        ya = a[:, 4].astype(np.float64)
        b[:, 0] = (b[:, 0] + t * np.cos(ya)).astype(np.float32)
        b[:, 1] = (b[:, 1] + t * np.sin(ya)).astype(np.float32)
        parts.append((a, b))
    a, b = _cat(*parts)
    A, B = a.astype(np.float64), b.astype(np.float64)
    ratio = np.hypot(A[:, 0] - B[:, 0], A[:, 1] - B[:, 1]) / np.minimum(A[:, 2:4].min(1), B[:, 2:4].min(1))
    want = iou64_pairs(a, b)
    assert (want > OVERLAP).mean() >= 0.95 and (ratio > 100).mean() >= 0.5 and (_aspect(a) > 1000).all()
    return a, b, want, BAR + SHIFT_TERM * ratio


# -------------------------------------------------------------------------------------------- decisions that went wrong
# Pairs drawn as the families "car, -100 turns against +100" and "barrier 12 x 0.3, A 100 turns ahead" (with centres in
# -50 ... -12, so that placed_case takes them) on which the arithmetic with w = yaw_a - yaw_b as ONE float32 subtraction was
# more than 3e-5 from the definition on the host: (a, b, float64 IoU, what that arithmetic gave).  In the NMS b sits in
# the earlier slot and a behind it: the operator evaluates iou(a, b).
FROZEN = (
    ((-44.458794, -27.142225, 5.0953507, 1.7686073, -629.41223), (-44.44441, -27.074625, 4.9626923, 1.6851325, 627.2164),
     0.9213030143559195, 0.9213441),            # +4.11e-05: the definition keeps a, that arithmetic suppressed it
    ((-41.930717, -33.762352, 13.1586485, 0.34598407, 628.3582), (-41.746334, -33.760277, 13.657045, 0.3594765, 0.040273402),
     0.9252977827813944, 0.9252252),            # -7.26e-05: the definition suppresses a, that arithmetic kept it
    ((-40.902016, -42.014076, 12.402242, 0.29492873, 626.2126), (-40.890785, -41.99682, 12.837186, 0.28624025, -2.1050746),
     0.9374871037663587, 0.93765396),           # +1.67e-04
)
FROZEN_GAP = 2e-5


def frozen_threshold(want, was):
    """2e-5 from the float64 IoU, on the side where the old arithmetic's value lay"""
    return want + FROZEN_GAP if was > want else want - FROZEN_GAP
