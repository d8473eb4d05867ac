"""Cases and the two oracles of bev_augment_boxes, shared by test_bev_augment_cpu.py (the host entry) and
test_bev_augment_gpu.py (the kernel).  Both oracles are numpy restatements of the definition in
accv-lab_amd/csrc/bev_augment_arith.h and share no code with the library.

Oracle (a), `oracle_a`: the float32 operation sequence, one IEEE operation per numpy operator, with a Python loop for the
compaction.  The operator must equal it exactly on every output tensor, padding and sizes included (`assert_same`; NaN
counts as equal to NaN at the same place, because the payload of a NaN is not part of the definition).

Oracle (b), `oracle_b`: a float64 evaluation of the reference's definition: A = T S R as 4 x 4 matrices with the cosine
and sine of the angle, M @ inv(A), A @ M, the yaw wrapped by a loop.  The bar per output tensor is n * 2^-24 * (the largest
magnitude among that tensor's float64 intermediates), n = the roundings on the longest chain of the definition, counting the
rounded constants c, s and 1/k: 5 for the boxes, 9 for the point transforms, 5 for the frame transforms (the header states
and derives the same numbers; test_bev_augment_cpu.py checks that they agree).  A yaw may differ by 0 or by 2π within the
bar, as in the reference's own test.
"""
import math

import numpy as np
import torch

N_BOX, N_POINT, N_FRAME = 5, 9, 5
U = 2.0 ** -24
F32 = np.float32
PI32, TWO_PI32 = F32(math.pi), F32(2.0 * math.pi)
THREADS = 256
IDENTITY = (0.0, 1.0, (0.0, 0.0, 0.0))


# ------------------------------------------------------------------------------------------------------------- inputs
def make_rows(params):
    """[B, 7] float32 rows from (angle, scale, (tx, ty, tz)) per frame: cos and sin in float64 from the float32 angle"""
    out = np.zeros((len(params), 7), F32)
    for b, (angle, scale, t) in enumerate(params):
        a = F32(angle)
        out[b] = (a, F32(math.cos(float(a))), F32(math.sin(float(a))), F32(scale), F32(t[0]), F32(t[1]), F32(t[2]))
    return out


class Case:
    """the inputs of one call, as numpy arrays"""

    def __init__(self, boxes, sizes, rows, labels=None, valid=None, point_range=None, on="input", pts=(), frs=(),
                 sizes_dtype=np.int64):
        self.boxes = np.ascontiguousarray(boxes, F32)
        self.sizes = np.asarray(sizes).astype(sizes_dtype)
        self.rows = np.ascontiguousarray(rows, F32)
        self.labels, self.valid, self.point_range, self.on = labels, valid, point_range, on
        self.pts = [np.ascontiguousarray(m, F32) for m in pts]
        self.frs = [np.ascontiguousarray(m, F32) for m in frs]


def fill_padding(boxes, sizes, lo=-40.0, hi=40.0):
    """padding slots get, in turn, NaN, 1e30 and a decoy that every range of these tests would keep"""
    fillers = (np.nan, 1e30, 0.5 * (lo + hi))
    for b, n in enumerate(sizes):
        for j in range(int(n), boxes.shape[1]):
            boxes[b, j] = fillers[(b + j) % 3]
    return boxes


def random_boxes(rng, B, N, D, xy=60.0):
    b = np.zeros((B, N, D), F32)
    b[..., 0:2] = rng.uniform(-xy, xy, (B, N, 2))
    b[..., 2] = rng.uniform(-6, 4, (B, N))
    b[..., 3:6] = rng.uniform(0.3, 12, (B, N, 3))
    b[..., 6] = rng.uniform(-math.pi, math.pi, (B, N))
    if D == 9:
        b[..., 7:9] = rng.uniform(-10, 10, (B, N, 2))
    return b


def random_params(rng, B):
    return [(rng.uniform(-math.pi, math.pi), rng.uniform(0.9, 1.1), tuple(rng.uniform(-2, 2, 3))) for _ in range(B)]


def random_poses(rng, B, K, rows=4, spread=2000.0):
    """rigid poses [B, K, rows, 4] with translations up to `spread` metres"""
    m = np.zeros((B, K, 4, 4))
    for b in range(B):
        for k in range(K):
            q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
            m[b, k, :3, :3] = q
            m[b, k, :3, 3] = rng.uniform(-spread, spread, 3)
            m[b, k, 3, 3] = 1.0
    return m[:, :, :rows].astype(F32)


# ----------------------------------------------------------------------------------------------------------- oracle (a)
def _wrap32(v):
    v = v.copy()
    low, high = v < -PI32, v > PI32
    v[low] = v[low] + np.ceil((-PI32 - v[low]) / TWO_PI32) * TWO_PI32
    v[high] = v[high] - np.ceil((v[high] - PI32) / TWO_PI32) * TWO_PI32
    return v


def _inside(point_range, x, y, z):
    """float32 coordinates against the Python numbers as given; NaN fails"""
    (lx, ly, lz), (hx, hy, hz) = point_range
    c = [np.asarray(v, np.float64) for v in (x, y, z)]
    return (lx <= c[0]) & (c[0] <= hx) & (ly <= c[1]) & (c[1] <= hy) & (lz <= c[2]) & (c[2] <= hz)


def oracle_a(case):
    boxes, rows = case.boxes, case.rows
    B, N, D = boxes.shape
    out = dict(boxes=np.zeros((B, N, D), F32), source=np.full((B, N), -1, np.int32), keep=np.zeros((B, N), bool),
               sizes=np.zeros((B,), np.int64), pts=[np.zeros_like(m) for m in case.pts], frs=[np.zeros_like(m) for m in case.frs],
               labels=None if case.labels is None else np.zeros_like(case.labels))
    with np.errstate(all="ignore"):
        for b in range(B):
            th, c, s, k, tx, ty, tz = (F32(v) for v in rows[b])
            size = int(min(max(int(case.sizes[b]), 0), N))
            bx = boxes[b, :size]
            x, y, z = bx[:, 0], bx[:, 1], bx[:, 2]
            ox = ((c * x - s * y) * k) + tx
            oy = ((s * x + c * y) * k) + ty
            oz = (z * k) + tz
            aug = np.zeros((size, D), F32)
            aug[:, 0], aug[:, 1], aug[:, 2] = ox, oy, oz
            aug[:, 3:6] = bx[:, 3:6] * k
            aug[:, 6] = _wrap32(bx[:, 6] + th)
            if D == 9:
                vx, vy = bx[:, 7], bx[:, 8]
                aug[:, 7] = (c * vx - s * vy) * k
                aug[:, 8] = (s * vx + c * vy) * k
            assert aug.dtype == F32
            on = np.ones((size,), bool) if case.valid is None else case.valid[b, :size] != 0
            if case.point_range is not None:
                on = on & (_inside(case.point_range, ox, oy, oz) if case.on == "output" else _inside(case.point_range, x, y, z))
            out["keep"][b, :size] = on
            kept = 0
            for n in range(size):          # the compaction, in slot order
                if on[n]:
                    out["boxes"][b, kept] = aug[n]
                    out["source"][b, kept] = n
                    if case.labels is not None:
                        out["labels"][b, kept] = case.labels[b, n]
                    kept += 1
            out["sizes"][b] = kept
            ik = F32(1.0) / k
            for m_in, m_out in zip(case.pts, out["pts"]):
                m = m_in[b]                # [K, R, 4]
                m0, m1, m2, m3 = m[..., 0], m[..., 1], m[..., 2], m[..., 3]
                r0 = m0 * c - m1 * s
                r1 = m0 * s + m1 * c
                q0, q1, q2 = r0 * ik, r1 * ik, m2 * ik
                u3 = m3 - ((q0 * tx + q1 * ty) + q2 * tz)
                m_out[b] = np.stack([q0, q1, q2, u3], -1)
            for m_in, m_out in zip(case.frs, out["frs"]):
                m = m_in[b]                # [K, 4, 4], columns along the last axis
                a0, a1, a2, a3 = m[:, 0], m[:, 1], m[:, 2], m[:, 3]
                m_out[b] = np.stack([((c * a0 - s * a1) * k) + tx * a3, ((s * a0 + c * a1) * k) + ty * a3, (a2 * k) + tz * a3, a3], 1)
    for v in out["pts"] + out["frs"]:
        assert v.dtype == F32
    return out


# ----------------------------------------------------------------------------------------------------------- oracle (b)
def _absmax(*arrays):
    m = 0.0
    for a in arrays:
        a = np.abs(np.asarray(a, np.float64))
        a = a[np.isfinite(a)]
        if a.size:
            m = max(m, float(a.max()))
    return m


def oracle_b(case):
    """float64 values of EVERY real input slot (no compaction; the caller gathers by oracle (a)'s source) and of every
    matrix, with the largest magnitude among the intermediates of each output tensor"""
    B, N, D = case.boxes.shape
    boxes = np.full((B, N, D), np.nan)
    pts = [np.zeros(m.shape) for m in case.pts]
    frs = [np.zeros(m.shape) for m in case.frs]
    mag = dict(boxes=0.0, pts=[0.0] * len(pts), frs=[0.0] * len(frs))
    with np.errstate(all="ignore"):
        for b in range(B):
            th, _, _, k, tx, ty, tz = (float(v) for v in case.rows[b])
            c, s = math.cos(th), math.sin(th)
            R = np.array([[c, -s, 0, 0], [s, c, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1.0]])
            S = np.diag([k, k, k, 1.0])
            T = np.eye(4)
            T[:3, 3] = (tx, ty, tz)
            A = T @ S @ R
            size = int(min(max(int(case.sizes[b]), 0), N))
            bx = case.boxes[b, :size].astype(np.float64)
            p = np.concatenate([bx[:, :3], np.ones((size, 1))], 1).T          # homogeneous columns
            rp, srp = R @ p, S @ R @ p
            boxes[b, :size, :3] = (A @ p)[:3].T
            boxes[b, :size, 3:6] = bx[:, 3:6] * k
            yaw = bx[:, 6] + th
            for i in range(size):
                v = yaw[i]
                if not math.isfinite(v):
                    v = math.nan
                while v < -math.pi:
                    v += 2.0 * math.pi
                while v > math.pi:
                    v -= 2.0 * math.pi
                boxes[b, i, 6] = v
            inter = [bx[:, :7], c * bx[:, :2], s * bx[:, :2], rp, srp, boxes[b, :size, :7], (tx, ty, tz), yaw]
            if D == 9:
                vel = np.concatenate([bx[:, 7:9], np.zeros((size, 2))], 1).T
                boxes[b, :size, 7:9] = (S @ R @ vel)[:2].T
                inter += [bx[:, 7:9], c * bx[:, 7:9], s * bx[:, 7:9], R @ vel, boxes[b, :size, 7:9]]
            mag["boxes"] = max(mag["boxes"], _absmax(*inter))
            inv = np.linalg.inv(A) if k != 0 and np.isfinite(A).all() else np.full((4, 4), np.nan)
            for i, m_in in enumerate(case.pts):
                m = m_in[b].astype(np.float64)
                pts[i][b] = m @ inv
                mag["pts"][i] = max(mag["pts"][i], _absmax(m, m @ R.T, m @ R.T @ np.linalg.inv(S) if k != 0 else 0.0,
                                                            m[..., :, None] * inv[None, None], pts[i][b]))
            for i, m_in in enumerate(case.frs):
                m = m_in[b].astype(np.float64)
                frs[i][b] = A @ m
                mag["frs"][i] = max(mag["frs"][i], _absmax(m, R @ m, S @ R @ m, A[None, :, :, None] * m[:, None], frs[i][b]))
    return dict(boxes=boxes, pts=pts, frs=frs, mag=mag)


# ------------------------------------------------------------------------------------------------------ run and compare
def to_torch(case, device, labels_dtype=torch.int64, valid_dtype=torch.bool, offset=False):
    """the arguments of bev_augment_boxes on `device`; with `offset`, boxes, params and the first matrix tensor are
    contiguous views that start one element into their storage"""
    from accvlab.batching_helpers import RaggedBatch

    def place(a, shifted):
        t = torch.from_numpy(np.ascontiguousarray(a))
        if not shifted:
            return t.to(device)
        buf = torch.empty((t.numel() + 1,), dtype=t.dtype, device=device)
        view = buf[1:].view(t.shape)
        view.copy_(t)
        assert view.storage_offset() == 1 and view.is_contiguous()
        return view

    sizes = torch.from_numpy(case.sizes).to(device)
    kw = dict(point_range=case.point_range, range_check_on=case.on,
              point_transforms=tuple(place(m, offset and i == 0) for i, m in enumerate(case.pts)),
              frame_transforms=tuple(place(m, False) for m in case.frs))
    if case.labels is not None:
        kw["labels"] = RaggedBatch(torch.from_numpy(case.labels).to(labels_dtype).to(device), sample_sizes=sizes)
    if case.valid is not None:
        kw["valid"] = torch.from_numpy(case.valid.astype(np.uint8)).to(valid_dtype).to(device)
    return RaggedBatch(place(case.boxes, offset), sample_sizes=sizes), place(case.rows, offset), kw


def _inputs(boxes, rows, kw):
    ts = [boxes.tensor, boxes.sample_sizes, rows, *kw["point_transforms"], *kw["frame_transforms"]]
    ts += [kw["labels"].tensor] if "labels" in kw else []
    ts += [kw["valid"]] if "valid" in kw else []
    return ts


def run(case, device, **how):
    """the operator's outputs as CPU tensors, in oracle (a)'s layout; the inputs must come back bit for bit"""
    from accvlab.draw_heatmap import bev_augment_boxes

    boxes, rows, kw = to_torch(case, device, **how)
    before = [t.clone() for t in _inputs(boxes, rows, kw)]
    out = bev_augment_boxes(boxes, rows, **kw)
    for a, b in zip(before, _inputs(boxes, rows, kw)):
        assert a.shape == b.shape and (a.numel() == 0 or torch.equal(a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8))), \
            "an input was modified"
    return flatten(out, case)


def flatten(out, case):
    assert out.boxes.sample_sizes is out.source.sample_sizes and out.boxes.sample_sizes.dtype == torch.int64
    assert (out.labels is None) == (case.labels is None)
    if out.labels is not None:
        assert out.labels.sample_sizes is out.boxes.sample_sizes
    assert out.keep.tensor.dtype == torch.bool and out.source.tensor.dtype == torch.int32
    assert torch.equal(out.keep.sample_sizes.cpu().to(torch.int64), torch.from_numpy(case.sizes.astype(np.int64)))
    return dict(boxes=out.boxes.tensor.cpu(), labels=None if out.labels is None else out.labels.tensor.cpu(),
                source=out.source.tensor.cpu(), keep=out.keep.tensor.cpu(), sizes=out.boxes.sample_sizes.cpu(),
                pts=[t.cpu() for t in out.point_transforms], frs=[t.cpu() for t in out.frame_transforms])


def same(a, b):
    """torch.equal, with NaN equal to NaN at the same place"""
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.is_floating_point():
        na, nb = a.isnan(), b.isnan()
        return torch.equal(na, nb) and torch.equal(torch.where(na, torch.zeros_like(a), a), torch.where(nb, torch.zeros_like(b), b))
    return torch.equal(a, b)


def _pairs(got, want):
    yield "boxes", got["boxes"], want["boxes"]
    yield "source", got["source"], want["source"]
    yield "keep", got["keep"], want["keep"]
    yield "sizes", got["sizes"], want["sizes"]
    if want["labels"] is not None:
        yield "labels", got["labels"], want["labels"]
    assert len(got["pts"]) == len(want["pts"]) and len(got["frs"]) == len(want["frs"])
    for i, (g, w) in enumerate(zip(got["pts"], want["pts"])):
        yield f"point_transforms[{i}]", g, w
    for i, (g, w) in enumerate(zip(got["frs"], want["frs"])):
        yield f"frame_transforms[{i}]", g, w


def assert_same(got, want, what=""):
    """every output tensor of `got` equals `want` (oracle (a) as numpy, or another run), padding and sizes included"""
    for name, g, w in _pairs(got, want):
        w = torch.from_numpy(np.ascontiguousarray(w)) if isinstance(w, np.ndarray) else w
        if name == "labels":
            w = w.to(g.dtype)
        assert same(g, w), f"{what} {name} differs"


def _ratio(got, ref, mag, n, yaw=None):
    """max |got - ref| / (2^-24 * mag) where ref is finite; got must be non-finite exactly where ref is"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    fin = np.isfinite(ref)
    assert np.array_equal(np.isfinite(got), fin), "finite values where the float64 evaluation has none, or the reverse"
    diff = np.abs(np.where(fin, got - ref, 0.0))
    if yaw is not None:
        diff[yaw] = np.minimum(diff[yaw], np.abs(diff[yaw] - 2.0 * math.pi))
    if mag == 0.0:
        assert not diff.any()
        return 0.0
    return float(diff.max() / (U * mag)) if diff.size else 0.0


def check_against_b(got, case, a=None, report=None, what=""):
    """`got` against the float64 evaluation, per output tensor, within n * 2^-24 * the tensor's largest intermediate; the
    kept boxes are found through oracle (a)'s source.  Returns the ratios error / (2^-24 * magnitude)."""
    a = a if a is not None else oracle_a(case)
    ref = oracle_b(case)
    B, N, D = case.boxes.shape
    g_rows, r_rows = [], []
    for b in range(B):
        for j in range(int(a["sizes"][b])):
            g_rows.append(got["boxes"][b, j].numpy())
            r_rows.append(ref["boxes"][b, a["source"][b, j]])
    ratios = {}
    if g_rows:
        yaw = np.zeros((len(g_rows), D), bool)
        yaw[:, 6] = True
        ratios["boxes"] = (_ratio(np.stack(g_rows), np.stack(r_rows), ref["mag"]["boxes"], N_BOX, yaw), N_BOX)
    for i, (g, r) in enumerate(zip(got["pts"], ref["pts"])):
        ratios[f"point_transforms[{i}]"] = (_ratio(g.numpy(), r, ref["mag"]["pts"][i], N_POINT), N_POINT)
    for i, (g, r) in enumerate(zip(got["frs"], ref["frs"])):
        ratios[f"frame_transforms[{i}]"] = (_ratio(g.numpy(), r, ref["mag"]["frs"][i], N_FRAME), N_FRAME)
    for name, (ratio, n) in ratios.items():
        line = f"{what} {name}: max error {ratio:.3f} x 2^-24 x largest intermediate (bar {n})"
        print(line)
        if report is not None:
            report.append(line)
    for name, (ratio, n) in ratios.items():
        assert ratio <= n, f"{what} {name}: {ratio:.3f} x 2^-24 x largest intermediate exceeds the bar of {n}"
    return ratios


# --------------------------------------------------------------------------------------------------------------- cases
def reference_case():
    """the data of the reference's bev_bboxes_transformer_3d_test.py:61-143 restated, one frame per parameter set:
    (π/2, 1.5, (0.5, 1, 1.5)), rotation only, translation only, everything off"""
    points = [[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 2, 3], [4, 5, 6], [7, 8, 9]]
    vel = [[0, 0], [1, 0], [0, 1], [0, 0], [0.1, 0.2], [0.4, 0.5], [0.7, 0.8]]
    sizes = [[1, 2, 3], [4, 5, 6], [7, 8, 9], [10, 11, 12], [2, 1.5, 1], [3, 2, 1.5], [2.5, 1.8, 1.2]]
    yaw = np.array([0.0, -np.pi + 0.0001, np.pi - 0.0001, -np.pi / 2, np.pi / 3, -np.pi / 6, np.pi], F32)
    frame = np.concatenate([np.array(points, F32), np.array(sizes, F32), yaw[:, None], np.array(vel, F32)], 1)
    ego = np.array([[1, 0, 0, 10], [0, 1, 0, 20], [0, 0, 1, 30], [0, 0, 0, 1]], F32)
    w2e = np.linalg.inv(ego).astype(F32)
    front = np.eye(4, dtype=F32)
    front[2, 3] = 100.0
    proj = np.array([[1000, 0, 320, 0], [0, 1000, 240, 0], [0, 0, 1, 0]], F32) @ front
    params = [(math.pi / 2, 1.5, (0.5, 1.0, 1.5)), (math.pi / 2, 1.0, (0, 0, 0)), (0.0, 1.0, (0.5, 1.0, 1.5)), IDENTITY]
    B = len(params)
    rep = lambda m: np.broadcast_to(m, (B, 1) + m.shape).copy()   # noqa: E731
    return Case(np.broadcast_to(frame, (B,) + frame.shape).copy(), [7] * B, make_rows(params), labels=np.tile(np.arange(7), (B, 1)),
                pts=[rep(proj), rep(ego)], frs=[rep(w2e)])


FRAME_SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 300)


def frame_sizes_case(D, keeps, seed=3):
    """frames of 0 .. 300 boxes in one batch, Nmax = 301; `keeps` is "all", "none" or "alternate" """
    rng = np.random.default_rng(seed)
    B, N = len(FRAME_SIZES), 301
    boxes = fill_padding(random_boxes(rng, B, N, D, xy=40.0), FRAME_SIZES)
    valid = {"all": None, "none": np.zeros((B, N), bool), "alternate": (np.arange(N)[None] + np.arange(B)[:, None]) % 2 == 0}[keeps]
    if valid is not None:
        valid = valid.copy()
        for b, n in enumerate(FRAME_SIZES):
            valid[b, n:] = True          # a padding slot that says "valid" is still padding
    return Case(boxes, FRAME_SIZES, make_rows(random_params(rng, B)), labels=rng.integers(-1, 10, (B, N)), valid=valid,
                point_range=((-50.0, -50.0, -10.0), (50.0, 50.0, 10.0)))


def _ulp_out(v, up):
    return float(np.nextafter(F32(v), F32(np.inf if up else -np.inf)))


BORDER_LO, BORDER_HI = (float(F32(-51.2)), float(F32(-51.2)), -5.0), (float(F32(51.2)), float(F32(51.2)), 3.0)


def range_border_case(on="input", inf_borders=False, double_border=False):
    """slots 0-5 on the six borders (kept), 6-11 one ulp outside them (dropped), 12-14 a NaN coordinate (dropped), 15 well
    inside (kept), 16 / 17 far out and infinite (kept only by infinite borders); identity rows, so "input" and "output"
    decide alike.  `double_border`: the borders are -51.2 / 51.2 as Python floats, which float32(±51.2) lies OUTSIDE of."""
    inside = [1.0, -2.0, 0.5]
    rows = []
    for axis in range(3):
        for v in (BORDER_LO[axis], BORDER_HI[axis]):
            rows.append([v if a == axis else inside[a] for a in range(3)])
    for axis in range(3):
        for v, up in ((BORDER_LO[axis], False), (BORDER_HI[axis], True)):
            rows.append([_ulp_out(v, up) if a == axis else inside[a] for a in range(3)])
    for axis in range(3):
        rows.append([np.nan if a == axis else inside[a] for a in range(3)])
    rows += [inside, [1e30, -1e30, 1e30], [np.inf, 0.0, -np.inf]]
    n = len(rows)
    boxes = np.zeros((2, n + 3, 7), F32)
    boxes[:, :n, :3] = np.array(rows, F32)
    boxes[:, :n, 3:6] = 1.0
    fill_padding(boxes, [n, n])
    rng = ((-math.inf,) * 3, (math.inf,) * 3) if inf_borders else ((-51.2, -51.2, -5.0), (51.2, 51.2, 3.0)) if double_border \
        else (BORDER_LO, BORDER_HI)
    return Case(boxes, [n, n], make_rows([IDENTITY, IDENTITY]), point_range=rng, on=on, sizes_dtype=np.int32)


def range_order_case(on):
    """a box inside before the augmentation and outside after it, one the other way round, one inside and one outside both
    times; x moves by +10"""
    boxes = np.zeros((1, 5, 9), F32)
    boxes[0, :4, 0] = (45.0, -55.0, 0.0, 70.0)
    boxes[0, :4, 3:6] = 2.0
    fill_padding(boxes, [4])
    return Case(boxes, [4], make_rows([(0.0, 1.0, (10.0, 0.0, 0.0))]), labels=np.arange(5)[None], point_range=(BORDER_LO, BORDER_HI), on=on)


def dtypes_case(seed=5):
    rng = np.random.default_rng(seed)
    B, N, sizes = 3, 70, [70, 0, 41]
    boxes = fill_padding(random_boxes(rng, B, N, 9), sizes)
    return Case(boxes, sizes, make_rows(random_params(rng, B)), labels=rng.integers(-1, 10, (B, N)), valid=rng.random((B, N)) < 0.7,
                point_range=((-51.2, -51.2, -5.0), (51.2, 51.2, 3.0)))


def yaw_case():
    yaws = [100.0, -100.0, float(PI32), -float(PI32), np.nan, np.inf, -np.inf, 3.0, -3.0, 0.0, 1000.0, -1000.0]
    B, n = 4, len(yaws)
    boxes = np.zeros((B, n, 7), F32)
    boxes[..., 3:6] = 1.0
    boxes[..., 6] = np.array(yaws, F32)
    return Case(boxes, [n] * B, make_rows([IDENTITY, (0.5, 1.0, (0, 0, 0)), (-0.5, 1.0, (0, 0, 0)), (math.pi, 1.0, (0, 0, 0))]))


def matrices_case(which, seed=7):
    """`which`: "k0" (K = 0), "mixed" (3 x 4 and 4 x 4 in one call), "full" (4 + 2 tensors, K = 70, a frame matrix whose
    last row is not (0, 0, 0, 1))"""
    rng = np.random.default_rng(seed)
    B, N, sizes = 3, 5, [5, 2, 0]
    boxes = fill_padding(random_boxes(rng, B, N, 7), sizes)
    rows = make_rows(random_params(rng, B))
    if which == "k0":
        pts, frs = [np.zeros((B, 0, 4, 4), F32), np.zeros((B, 0, 3, 4), F32)], [np.zeros((B, 0, 4, 4), F32)]
    elif which == "mixed":
        pts, frs = [random_poses(rng, B, 6, rows=3), random_poses(rng, B, 6)], []
    else:
        general = rng.uniform(-3, 3, (B, 1, 4, 4)).astype(F32)      # projective: the last row is anything
        pts = [random_poses(rng, B, 6), random_poses(rng, B, 6, rows=3), random_poses(rng, B, 70), np.zeros((B, 0, 4, 4), F32)]
        frs = [general, random_poses(rng, B, 70)]
    return Case(boxes, sizes, rows, pts=pts, frs=frs)


def empty_case(which):
    rng = np.random.default_rng(11)
    if which == "B0":
        return Case(np.zeros((0, 4, 9), F32), [], np.zeros((0, 7), F32), labels=np.zeros((0, 4), np.int64),
                    pts=[np.zeros((0, 2, 4, 4), F32)], frs=[np.zeros((0, 1, 4, 4), F32)])
    B = 2          # Nmax = 0: the matrices and the sizes are still written
    return Case(np.zeros((B, 0, 7), F32), [0, 0], make_rows(random_params(rng, B)), labels=np.zeros((B, 0), np.int64),
                valid=np.zeros((B, 0), bool), point_range=(BORDER_LO, BORDER_HI), pts=[random_poses(rng, B, 2)], frs=[random_poses(rng, B, 1)])


SWEEP_RANGE = ((-51.2, -51.2, -5.0), (51.2, 51.2, 3.0))


def sweep_case(seed, on="input"):
    """nuScenes-like frames: centres uniform in [-70, 70]^2 x [-6, 4], valid true at 0.9, six cameras, ego poses with
    translations up to 2000 m"""
    rng = np.random.default_rng(seed)
    B, N = 6, 120
    sizes = rng.integers(40, N + 1, B)
    boxes = random_boxes(rng, B, N, 9)
    boxes[..., 0:2] = rng.uniform(-70, 70, (B, N, 2))
    fill_padding(boxes, sizes)
    return Case(boxes, sizes, make_rows(random_params(rng, B)), labels=rng.integers(0, 10, (B, N)), valid=rng.random((B, N)) < 0.9,
                point_range=SWEEP_RANGE, on=on, pts=[random_poses(rng, B, 6, spread=3.0), random_poses(rng, B, 1)],
                frs=[np.linalg.inv(random_poses(rng, B, 1).astype(np.float64)).astype(F32)])


def sweep_shares(case, a):
    real = int(sum(min(int(s), case.boxes.shape[1]) for s in case.sizes))
    kept = int(a["sizes"].sum())
    return kept / real, (real - kept) / real


CASES = {
    "reference": reference_case,
    **{f"sizes-D{D}-{keeps}": (lambda D=D, keeps=keeps: frame_sizes_case(D, keeps)) for D in (7, 9) for keeps in ("all", "none", "alternate")},
    "borders-input": lambda: range_border_case("input"),
    "borders-output": lambda: range_border_case("output"),
    "borders-inf": lambda: range_border_case(inf_borders=True),
    "borders-double": lambda: range_border_case(double_border=True),
    "order-input": lambda: range_order_case("input"),
    "order-output": lambda: range_order_case("output"),
    "dtypes": dtypes_case,
    "yaw": yaw_case,
    "matrices-k0": lambda: matrices_case("k0"),
    "matrices-mixed": lambda: matrices_case("mixed"),
    "matrices-full": lambda: matrices_case("full"),
    "empty-B0": lambda: empty_case("B0"),
    "empty-N0": lambda: empty_case("N0"),
    "sweep-1-input": lambda: sweep_case(1, "input"),
    "sweep-2-output": lambda: sweep_case(2, "output"),
}
# the cases whose real boxes and matrices are finite numbers of ordinary size (and the yaws, where the float64 evaluation
# turns non-finite ones into NaN as the definition does): compared with oracle (b) too
B_CASES = {n for n in CASES if not n.startswith(("borders", "empty"))}
_BUILT = {}


def built(name):
    """(case, oracle (a)) of a named case, computed once per process and never modified"""
    if name not in _BUILT:
        case = CASES[name]()
        _BUILT[name] = (case, oracle_a(case))
    return _BUILT[name]


def check_case(name, device, report=None, **how):
    """the operator on `device` equals oracle (a) on every output, and lies within the bar of oracle (b)"""
    case, a = built(name)
    got = run(case, device, **how)
    assert_same(got, a, f"{name} on {device}:")
    if name in B_CASES:
        check_against_b(got, case, a, report=report, what=f"{name} on {device}:")
    return case, a, got


CPT = dict(pc_range=[-51.2, -51.2, -5.0, 51.2, 51.2, 3.0], voxel_size=[0.2, 0.2, 8.0], out_size_factor=8, grid_size=(64, 64),
           gaussian_overlap=0.1, min_radius=2, max_objs=500, norm_bbox=True)
CPT_TASKS = ((0,), (1, 2), (3, 4), (5,), (6, 7), (8, 9))


def check_end_to_end(name, device):
    """center_point_targets on the operator's output equals center_point_targets on oracle (a)'s output"""
    from accvlab.batching_helpers import RaggedBatch
    from accvlab.draw_heatmap import bev_augment_boxes, center_point_targets

    case, a = built(name)
    boxes, rows, kw = to_torch(case, device)
    out = bev_augment_boxes(boxes, rows, **kw)
    got = center_point_targets(out.boxes, out.labels, CPT_TASKS, **CPT)
    sizes = torch.from_numpy(a["sizes"]).to(device)
    want = center_point_targets(RaggedBatch(torch.from_numpy(a["boxes"]).to(device), sample_sizes=sizes),
                                RaggedBatch(torch.from_numpy(a["labels"]).to(device), sample_sizes=sizes), CPT_TASKS, **CPT)
    assert sum(int(t.centers.sample_sizes.sum()) for t in want) > 50
    for t, (g, w) in enumerate(zip(got, want)):
        for field in g._fields:
            assert torch.equal(getattr(g, field).tensor, getattr(w, field).tensor), f"task {t} {field}"
        assert torch.equal(g.centers.sample_sizes, w.centers.sample_sizes)


def check_guard_bands(name, device, labels, trampoline=False):
    """the C entry alone (plain ctypes, or the trampoline the operators use) on sentinel-filled outputs between guard
    bands: nothing outside is touched, and everything inside is written (it equals oracle (a), padding included)"""
    import ctypes

    from accvlab import _amd_native as nat

    case, a = built(name)
    boxes, rows, kw = to_torch(case, device)
    B, N, D = case.boxes.shape
    pad = 512

    def banded(shape, dtype):
        nbytes = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        buf = torch.full((pad + nbytes + pad,), 0xA5, dtype=torch.uint8, device=device)   # the sentinel fills the inside too
        return buf, buf[pad: pad + nbytes].view(dtype).view(shape)

    lab = kw["labels"].tensor if labels else None
    bands = dict(boxes=banded((B, N, D), torch.float32), source=banded((B, N), torch.int32), keep=banded((B, N), torch.bool),
                 sizes=banded((B,), torch.int64))
    if labels:
        bands["labels"] = banded((B, N), torch.int64)
    for i, m in enumerate(kw["point_transforms"]):
        bands[f"pts{i}"] = banded(tuple(m.shape), torch.float32)
    for i, m in enumerate(kw["frame_transforms"]):
        bands[f"frs{i}"] = banded(tuple(m.shape), torch.float32)
    p = nat.BevAugmentParams()
    if case.point_range is not None:
        for c in range(3):
            p.range_min[c], p.range_max[c] = case.point_range[0][c], case.point_range[1][c]
        p.has_range = 1
    for i, m in enumerate(kw["point_transforms"]):
        p.point_in[i], p.point_out[i], p.point_count[i], p.point_rows[i] = m.data_ptr(), bands[f"pts{i}"][1].data_ptr(), m.shape[1], m.shape[2]
    for i, m in enumerate(kw["frame_transforms"]):
        p.frame_in[i], p.frame_out[i], p.frame_count[i] = m.data_ptr(), bands[f"frs{i}"][1].data_ptr(), m.shape[1]
    p.num_point_transforms, p.num_frame_transforms = len(case.pts), len(case.frs)
    flags = (nat.BA_COUNTS_I64 if case.sizes.dtype == np.int64 else 0) | (nat.BA_LABELS_I64 if labels else 0) | (nat.BA_RANGE_ON_OUTPUT if case.on == "output" else 0)
    valid = kw["valid"].data_ptr() if "valid" in kw else None
    args = (boxes.tensor.data_ptr(), rows.data_ptr(), lab.data_ptr() if labels else None, valid, boxes.sample_sizes.data_ptr(), flags,
            B, N, D, ctypes.addressof(p), bands["boxes"][1].data_ptr(), bands["labels"][1].data_ptr() if labels else None,
            bands["source"][1].data_ptr(), bands["keep"][1].data_ptr(), bands["sizes"][1].data_ptr())
    lib = nat.lib() if trampoline else nat.ctypes_lib()
    if torch.device(device).type == "cuda":
        status = lib.accv_bev_augment(*args, nat.stream_ptr(torch.device("cuda", torch.cuda.current_device())))
        torch.cuda.synchronize()
    else:
        status = lib.accv_bev_augment_host(*args)
    assert status == 0, nat.ctypes_lib().accv_last_error()
    for key, (buf, inner) in bands.items():
        n = inner.numel() * inner.element_size()
        assert bool((buf[:pad] == 0xA5).all()) and bool((buf[pad + n:] == 0xA5).all()), f"{key}: wrote outside its buffer"
    got = dict(boxes=bands["boxes"][1].cpu(), labels=bands["labels"][1].cpu() if labels else None, source=bands["source"][1].cpu(),
               keep=bands["keep"][1].cpu(), sizes=bands["sizes"][1].cpu(), pts=[bands[f"pts{i}"][1].cpu() for i in range(len(case.pts))],
               frs=[bands[f"frs{i}"][1].cpu() for i in range(len(case.frs))])
    want = dict(a)
    if not labels:
        want["labels"] = None
    # without labels the operator is told of none, and an oracle run without them decides alike
    assert_same(got, want, f"{name} banded:")
