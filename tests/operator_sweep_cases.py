"""Seeded random draws for the sweeps of the matching, loss and detection operators (test_operator_sweeps_cpu.py,
test_operator_sweeps_gpu.py).

One function per operator: ``draw_<operator>(rng, device="cpu") -> (inputs, kwargs, description)``.  Every draw is a pure
function of the numpy generator: the seed of the generator and the number of draws taken from it reproduce a case, and
`description` names every drawn parameter for the failure message.  The inputs come from the ``make_case`` builders of the
operators' own ``*_cases.py`` modules (seeded from `rng`); what is drawn here is what those builders take as arguments.

Every value list straddles a constant of the operator's kernel (wave 64, chunk or workgroup 256, tiles of 64 / 128 / 256,
the column tile of 2048, kMaxQ = 1024): the smallest shapes at which the kernel takes another path.  Where the float64
definition is a Python loop, the batch size is cut so that a case stays within a fraction of a second on the CPU; the
cut keeps the drawn edge (Q, K, N) and lowers B.
"""
import math

import numpy as np
import torch

FLOATS4 = [torch.float32, torch.float16, torch.bfloat16, torch.float64]
FLOATS3 = [torch.float32, torch.float16, torch.bfloat16]
INTS = [torch.int32, torch.int64]
name = lambda d: str(d).split(".")[-1]   # noqa: E731
# redraws of a case whose comparison sat on a threshold, per operator (the tests assert their share)
REDRAWS = {"center_point_decode": 0}


def pick(rng, values):
    return values[int(rng.integers(0, len(values)))]


def seed_of(rng):
    return int(rng.integers(0, 2 ** 31 - 1))


def ragged_sizes(rng, B, hi):
    """B sizes in [0, hi]: one frame full, and (B >= 3) a frame of size 0 that is neither the first nor the last"""
    sizes = [int(v) for v in rng.integers(0, hi + 1, size=B)]
    sizes[0 if rng.integers(0, 2) else B - 1] = hi
    if B >= 3:
        sizes[int(rng.integers(1, B - 1))] = 0
    return sizes


def pairs_within(rng, sizes, Q):
    """pairs per frame: everything matched, or a random part of it"""
    full = bool(rng.integers(0, 2))
    return [min(s, Q) if full else int(rng.integers(0, min(s, Q) + 1)) for s in sizes]


# ------------------------------------------------------------------------------------------------------ the loss side
def draw_matched_focal_loss(rng, device="cpu"):
    from matched_focal_loss_cases import make_case

    B = int(rng.integers(1, 7))
    C = pick(rng, [1, 2, 3, 5, 8, 10, 17, 80, 91, 513])
    Q = pick(rng, [1, 5, 33] if C >= 100 else [1, 5, 64, 100, 300, 900, 1030])
    dtype, index_dtype, label_dtype = pick(rng, FLOATS4), pick(rng, INTS), pick(rng, INTS)
    width = C + int(rng.integers(1, 9)) if rng.integers(0, 2) else None
    sigma = pick(rng, [1.0, 4.0, 8.0, 16.0])
    weights = bool(rng.integers(0, 2))
    sizes = ragged_sizes(rng, B, min(Q, pick(rng, [1, 6, 40, 100])))
    n_pairs = pairs_within(rng, sizes, Q)
    seed = seed_of(rng)
    kw = dict(alpha=pick(rng, [0.25, 0.5, -1.0]), gamma=pick(rng, [0.0, 1.0, 1.5, 2.0]))
    if rng.integers(0, 3) == 0:
        kw["avg_factor"] = 3.7
    inp = make_case(B, Q, C, sizes, n_pairs, dtype, seed=seed, index_dtype=index_dtype, label_dtype=label_dtype, device=device,
                    width=width, sigma=sigma, weights=weights)
    what = (f"matched_focal_loss B {B} Q {Q} C {C} {name(dtype)} width {width} sigma {sigma} weights {weights} sizes {sizes} "
            f"pairs {n_pairs} idx {name(index_dtype)} labels {name(label_dtype)} builder seed {seed} {kw}")
    return inp, kw, what


def draw_matched_box_loss(rng, device="cpu"):
    from matched_box_loss_cases import make_case

    B = int(rng.integers(1, 7))
    Q = pick(rng, [1, 2, 7, 63, 64, 65, 255, 256, 257, 300, 700])
    D = pick(rng, [4, 7, 10])
    dtype, index_dtype = pick(rng, FLOATS4), pick(rng, INTS)
    box_format = pick(rng, ["xyxy", "cxcywh"])
    iou_kind = pick(rng, [None, "iou", "giou"]) if D == 4 else None
    width = D + int(rng.integers(1, 6)) if rng.integers(0, 2) else None
    offset = int(rng.integers(0, 4))
    weights = bool(rng.integers(0, 2))
    sizes = ragged_sizes(rng, B, min(Q, pick(rng, [1, 6, 40, 100])))
    n_pairs = pairs_within(rng, sizes, Q)
    seed = seed_of(rng)
    kw = dict(box_format=box_format, iou_kind=iou_kind)
    if rng.integers(0, 2):
        cw = np.round(rng.random(D) * 2.0, 3)
        cw[rng.random(D) < 0.2] = 0.0
        kw["code_weights"] = [float(v) for v in cw]
    if rng.integers(0, 3) == 0:
        kw["avg_factor"] = 3.7
    inp = make_case(B, Q, D, sizes, n_pairs, dtype, seed=seed, box_format=box_format, index_dtype=index_dtype, device=device,
                    width=width, weights=weights, offset=offset)
    what = (f"matched_box_loss B {B} Q {Q} D {D} {name(dtype)} width {width} offset {offset} weights {weights} sizes {sizes} "
            f"pairs {n_pairs} idx {name(index_dtype)} builder seed {seed} {kw}")
    return inp, kw, what


def draw_batched_matching_cost(rng, device="cpu"):
    from matching_cost_cases import BOX_TERMS, KINDS, make_case, term_kwargs

    B = int(rng.integers(1, 7))
    G = pick(rng, [1, 3, 63, 64, 65, 130, 257])
    Q = pick(rng, [1, 7, 33, 100])
    C = pick(rng, [1, 4, 11, 92])
    kind, box_terms = pick(rng, KINDS), pick(rng, sorted(BOX_TERMS))
    dtype, label_dtype = pick(rng, FLOATS4), pick(rng, INTS)
    kw, D = term_kwargs(kind, box_terms)
    width = D + 3 if rng.integers(0, 2) else None
    if rng.integers(0, 3) == 0:
        kw["filler"] = -7.25
    sizes = ragged_sizes(rng, B, G)
    seed = seed_of(rng)
    inp = make_case(B, Q, C, sizes, kind, D, kw["box_format"], dtype, seed=seed, label_dtype=label_dtype, device=device, width=width)
    what = (f"batched_matching_cost B {B} Q {Q} C {C} G {G} sizes {sizes} {kind}/{box_terms} {name(dtype)} width {width} "
            f"labels {name(label_dtype)} builder seed {seed} filler {kw.get('filler', 0.0)}")
    return inp, kw, what


def draw_polyline(rng, device="cpu"):
    """one case for batched_polyline_matching_cost and matched_polyline_loss; kwargs holds `loss` and `cost`"""
    from polyline_match_cases import make_case

    B = int(rng.integers(1, 7))
    P, D = pick(rng, [2, 3, 5, 20, 33]), pick(rng, [2, 3])
    Q = pick(rng, [1, 6, 63, 65, 130])
    G = pick(rng, [1, 3, 7, 65])
    closed, reversible = pick(rng, ["open", "closed", "mixed"]), bool(rng.integers(0, 2))
    dtype, index_dtype = pick(rng, FLOATS4), pick(rng, INTS)
    closed_dtype = pick(rng, [torch.bool, torch.uint8, torch.int32, torch.int64])
    width = P * D + 3 if rng.integers(0, 2) else None
    # the cost definition gathers [Q, V, P, D] per ground-truth line in a Python loop: keep B G Q V P D near 2e7
    V = (1 if closed == "open" else P) * (2 if reversible else 1)
    while B > 1 and B * G * Q * V * P * D > 2e7:
        B -= 1
    while G > 3 and B * G * Q * V * P * D > 2e7:
        G = {65: 7, 7: 3}[G]
    sizes = ragged_sizes(rng, B, G)
    n_pairs = pairs_within(rng, sizes, Q)
    seed = seed_of(rng)
    loss = dict(reversible=reversible, dir_loss=bool(rng.integers(0, 4) > 0))
    if rng.integers(0, 3) == 0:
        loss["avg_factor"] = 3.7
    cost = dict(reversible=reversible, pts_weight=pick(rng, [1.0, 1.5]), filler=pick(rng, [0.0, -7.25]))
    inp = make_case(B, Q, P, D, sizes, n_pairs, dtype, seed=seed, closed=closed, reversible=reversible, index_dtype=index_dtype,
                    closed_dtype=closed_dtype, device=device, width=width)
    what = (f"polyline B {B} Q {Q} P {P} D {D} G {G} sizes {sizes} pairs {n_pairs} {closed} reversible {reversible} {name(dtype)} "
            f"width {width} idx {name(index_dtype)} closed as {name(closed_dtype)} builder seed {seed} loss {loss} cost {cost}")
    return inp, dict(loss=loss, cost=cost), what


# ------------------------------------------------------------------------------------------------- the detection side
DECODE_TASKS = {1: ((3, 0, 7),), 2: ((5, 2), (7,))}


def _off_the_score_threshold(case, threshold):
    """moves every logit score whose float64 sigmoid lies within 2 MARGIN of `threshold` up by 0.02 (at least one
    representable step of its dtype): sigmoid' = 0.09 at 0.1, so the score moves by 1.8e-3.  -> whether every score of
    the case is now further than 2 MARGIN away"""
    from center_decode_cases import MARGIN

    clear = True
    for s, _, _ in case.peaks:
        near = (torch.sigmoid(s.double()) - threshold).abs() <= 2 * MARGIN
        if bool(near.any()):
            s.copy_(torch.where(near, (s.double() + 0.02).to(s.dtype), s))     # logits lie in (-4, 4): spacing <= 0.0157
        clear = clear and not bool(((torch.sigmoid(s.double()) - threshold).abs() <= 2 * MARGIN).any())
    return clear


def draw_center_point_decode(rng, device="cpu"):
    """inputs: a center_decode_cases.Case on the host (the GPU test moves it); kwargs holds `cfg` and `options`.  With logit
    scores and a score threshold the comparison is only meaningful off the threshold (center_decode_cases.assert_margin):
    among up to 36 000 sigmoid scores some always come within 1e-4 of 0.1, so the draw moves those off it; a case that still
    has one is drawn again from the next builder seed and counted in REDRAWS."""
    from center_decode_cases import NUSC, NUSC_RANGE, NUSC_TASKS, make_case

    K = pick(rng, [1, 63, 64, 65, 255, 256, 257, 500, 1024])
    C = pick(rng, [8, 10])
    T = pick(rng, [1, 2, 6])
    tasks = NUSC_TASKS if T == 6 else DECODE_TASKS[T]
    B = max(1, min(int(rng.integers(1, 7)), 4096 // (K * T)))      # the definition is a loop over B T K peaks
    dtype = pick(rng, FLOATS3)
    score_dtype = pick(rng, [None, torch.float32])
    logits = bool(rng.integers(0, 2))
    opt = dict(norm_bbox=bool(rng.integers(0, 2)), bottom_center=bool(rng.integers(0, 2)))
    if logits:
        opt["scores_are_logits"] = True
    if rng.integers(0, 2):
        opt["post_center_range"] = NUSC_RANGE
    nms = pick(rng, [None, 0.2, 1.0, 4.0, 30.0])
    if nms is not None:
        opt["nms_threshold"] = [nms if (t + int(nms)) % 3 else None for t in range(T)] if T > 1 and rng.integers(0, 2) else nms
    post = pick(rng, [None, 1, 40, 83, 300])
    if post is not None:
        opt["post_max_size"] = post
    if rng.integers(0, 2):
        opt["score_threshold"] = 0.1
    seed = seed_of(rng)
    for attempt in range(10):
        case = make_case(B, K, tasks, C=C, dtype=dtype, score_dtype=score_dtype, seed=seed + attempt, logits=logits, device="cpu")
        if not (logits and "score_threshold" in opt) or _off_the_score_threshold(case, opt["score_threshold"]):
            break
        REDRAWS["center_point_decode"] += 1
    else:
        raise AssertionError("ten builder seeds in a row left a score on the threshold: the draw is broken")
    what = (f"center_point_decode B {B} K {K} C {C} tasks {T} maps {name(dtype)} scores {name(score_dtype or dtype)} "
            f"builder seed {seed + attempt} {opt}")
    return case, dict(cfg=NUSC, options=opt), what


def draw_rotated_nms_bev(rng, device="cpu"):
    """inputs: a rotated_nms_cases.Case on the host with its float64 IoU matrices; kwargs holds `thresholds` (chosen by
    pick_threshold, None for a task without NMS) and `options`"""
    import rotated_nms_cases as rn

    N = pick(rng, [1, 63, 65, 200, 257, 600])
    D = pick(rng, [7, 9])
    T = int(rng.integers(1, 4))
    B = int(rng.integers(1, 7))
    while B * T > 1 and B * T * N * N > 4e5:          # the float64 IoU clips every near pair
        B, T = (B - 1, T) if B > 1 else (B, T - 1)
    sizes = ragged_sizes(rng, B, N)
    seed = seed_of(rng)
    bevs, ious = rn._frames.__wrapped__(B, N, T, seed)      # not through the builder's cache: every draw is new
    task_rng = np.random.default_rng(seed + D)
    case = rn.Case([rn._task(bev, D, task_rng, sizes) for bev in bevs], ious)
    starts = [0.2, 0.5, 0.05]
    none_at = int(rng.integers(0, T + 2))             # one task without a threshold in some cases
    thr = [None if t == none_at and T > 1 else rn.pick_threshold(case, t, starts[t]) for t in range(T)]
    opt = {}
    pre, post = pick(rng, [None, 1, 64, 100, 500]), pick(rng, [None, 1, 40, 83])
    if pre is not None:
        opt["pre_max_size"] = pre
    if post is not None:
        opt["post_max_size"] = post
    what = f"rotated_nms_bev B {B} N {N} D {D} tasks {T} sizes {sizes} thresholds {thr} builder seed {seed} {opt}"
    return case, dict(thresholds=thr, options=opt), what


def draw_center_point_targets(rng, device="cpu"):
    """inputs: (boxes, labels) RaggedBatch on `device`; kwargs holds `tasks`, `cfg` and `options`"""
    from center_targets_cases import NUSC, NUSC_TASKS, make_case

    N = pick(rng, [0, 1, 63, 65, 257, 513])
    D = pick(rng, [7, 9])
    T = pick(rng, [1, 2, 6])
    tasks = NUSC_TASKS if T == 6 else DECODE_TASKS[T]
    B = max(1, min(int(rng.integers(1, 7)), 3000 // max(N * T, 1)))    # the definition is a loop over B T N objects
    sizes = ragged_sizes(rng, B, N)
    label_dtype, size_dtype = pick(rng, INTS), pick(rng, INTS)
    opt = dict(max_objs=pick(rng, [10, 100, 500]), norm_bbox=bool(rng.integers(0, 2)))
    seed = seed_of(rng)
    boxes, labels = make_case(B, N, sizes, D=D, seed=seed, label_dtype=label_dtype, size_dtype=size_dtype, device=device)
    what = (f"center_point_targets B {B} N {N} D {D} tasks {T} sizes {sizes} labels {name(label_dtype)} sizes as {name(size_dtype)} "
            f"builder seed {seed} {opt}")
    return (boxes, labels), dict(tasks=tasks, cfg=NUSC, options=opt), what


# ---------------------------------------------------------------------------------------------------------- assignment
def draw_batched_linear_sum_assignment(rng, device="cpu"):
    """inputs: the cost (a tensor or a RaggedBatch over rows or columns) on `device`; kwargs: maximize, _threads"""
    from accvlab.batching_helpers import RaggedBatch

    R = pick(rng, [1, 2, 9, 64, 65, 257, 300])
    C = pick(rng, [1, 3, 20, 64, 100, 256, 257])
    B = int(rng.integers(1, 7))
    dtype = pick(rng, FLOATS4)
    dist = pick(rng, ["uniform", "ties", "normal"])
    maximize = bool(rng.integers(0, 2))
    forbid = bool(rng.integers(0, 5) == 0)
    form = pick(rng, ["dense", "rows", "columns"])
    threads = pick(rng, [None, 64, 1024])
    if dist == "uniform":
        cost = rng.random((B, R, C))
    elif dist == "ties":
        cost = rng.integers(0, 4, (B, R, C)).astype(np.float64)
    else:
        cost = rng.normal(0.0, 100.0, (B, R, C))
    if forbid:
        cost[rng.random((B, R, C)) < 0.1] = -np.inf if maximize else np.inf
    t = torch.from_numpy(cost).to(dtype).to(device)
    sizes = None
    if form != "dense":
        sizes = ragged_sizes(rng, B, R if form == "rows" else C)
        t = RaggedBatch(t, sample_sizes=torch.tensor(sizes, dtype=torch.int64, device=device), non_uniform_dim=1 if form == "rows" else 2)
    kw = dict(maximize=maximize, _threads=threads)
    what = f"batched_linear_sum_assignment B {B} R {R} C {C} {name(dtype)} {dist} forbidden {forbid} {form} sizes {sizes} {kw}"
    return t, kw, what


def assignment_frames(cost):
    """the float64 matrices of the frames of a drawn cost, on the host"""
    if hasattr(cost, "tensor"):
        t, sizes, dim = cost.tensor.cpu().double(), cost.sample_sizes.cpu().tolist(), cost.non_uniform_dim
        return [(t[b, :n] if dim == 1 else t[b, :, :n]).numpy() for b, n in enumerate(sizes)]
    return [m.numpy() for m in cost.cpu().double()]


def check_assignment_against_scipy(result, cost, maximize, what):
    """per frame: status 1 and size 0 where scipy calls the matrix infeasible; otherwise status 0, min(rows, columns)
    pairs with distinct, ascending rows and distinct columns, and scipy's total cost on the float64 matrix (rtol 1e-12)"""
    from scipy.optimize import linear_sum_assignment

    rows, cols, status = result
    n = rows.sample_sizes.cpu().tolist()
    assert cols.sample_sizes.cpu().tolist() == n, what
    r_all, c_all, st = rows.tensor.cpu().numpy(), cols.tensor.cpu().numpy(), status.cpu().tolist()
    for b, m in enumerate(assignment_frames(cost)):
        try:
            er, ec = linear_sum_assignment(m, maximize=maximize)
        except ValueError as e:
            assert "infeasible" in str(e), f"{what} frame {b}: scipy says {e}"
            assert st[b] == 1 and n[b] == 0, f"{what} frame {b}: infeasible for scipy, status {st[b]} size {n[b]}"
            continue
        assert st[b] == 0 and n[b] == min(m.shape), f"{what} frame {b}: status {st[b]} size {n[b]} for a {m.shape} matrix"
        r, c = r_all[b, :n[b]], c_all[b, :n[b]]
        assert (np.diff(r) > 0).all() and len(set(c.tolist())) == n[b] and (r >= 0).all() and (r < m.shape[0]).all() \
            and (c >= 0).all() and (c < m.shape[1]).all(), f"{what} frame {b}: not a matching"
        got, want = float(m[r, c].sum()), float(m[er, ec].sum())
        assert abs(got - want) <= 1e-12 * abs(want), f"{what} frame {b}: total cost {got!r}, scipy {want!r}"


# ------------------------------------------------------------------------------------- the operators without a host path
def draw_heatmap_peaks(rng, device="cpu"):
    """inputs: the heat map on `device`; kwargs: k, kernel, per_class"""
    H = pick(rng, [1, 2, 7, 33, 65])
    W = pick(rng, [1, 3, 64, 130, 2047, 2048, 2049, 2500])
    C = pick(rng, [1, 3])
    B = max(1, min(int(rng.integers(1, 7)), 600000 // (C * H * W)))
    dtype = pick(rng, FLOATS3)
    per_class = bool(rng.integers(0, 2))
    group = H * W * (1 if per_class else C)
    k = min(pick(rng, [1, 7, 100, 1024]), group, 1024)
    kernel = pick(rng, [1, 3, 5, 7])
    values = pick(rng, ["normal", "levels", "negative"])
    shape = (B, H, W) if C == 1 and rng.integers(0, 2) else (B, C, H, W)
    if values == "normal":
        x = rng.standard_normal(shape)
    elif values == "levels":
        x = rng.integers(0, 4, shape) * 0.25
    else:
        x = -(rng.random(shape) + 0.1)
    heat = torch.from_numpy(np.ascontiguousarray(x)).to(dtype).to(device)
    kw = dict(k=k, kernel=kernel, per_class=per_class)
    return heat, kw, f"heatmap_peaks {shape} {name(dtype)} {values} {kw}"


def peaks_definition(heat, k, kernel=3, per_class=False, dtype=torch.float64):
    """test_heatmap_peaks_gpu.reference evaluated in `dtype` (float64: the same function, checked by the CPU sweep)"""
    import torch.nn.functional as F

    x = heat.detach().cpu().to(dtype)
    x4 = x if x.dim() == 4 else x.unsqueeze(1)
    B, C, H, W = x4.shape
    hmax = F.max_pool2d(x4, kernel, stride=1, padding=(kernel - 1) // 2)
    s = x4 * (hmax == x4)
    flat = s.reshape(B * C, H * W) if per_class else s.reshape(B, C * H * W)
    sc, order = torch.sort(flat, dim=1, descending=True, stable=True)
    sc, order = sc[:, :k], order[:, :k]
    if per_class:
        cls, inds = torch.arange(C).repeat(B).unsqueeze(1).expand(-1, k), order
    else:
        cls, inds = order // (H * W), order % (H * W)
    out = (sc.to(heat.dtype), inds, cls.contiguous(), inds // W, inds % W)
    return tuple(t.reshape(B, C, k) for t in out) if per_class else out


FOCAL_SHAPES = [(1, 1, 7), (3, 5, 9), (2, 33, 65), (2, 3, 37, 53), (1, 10, 37, 53), (4, 67, 129), (2, 270, 479), (1, 3, 271, 367)]


def draw_gaussian_focal_loss(rng, device="cpu"):
    """inputs: (logits, target) on `device`, both contiguous, both 0 or 4 bytes off their allocation's alignment; the
    target is drawn by the CPU oracle of draw_heatmap_batched on random objects (centres inside the map: every object puts
    an exact 1 there).  Logits are bounded by 10 (the definition adds 1e-12 inside its logarithms)."""
    import bench_workloads as wl
    from oracle import h1

    shape = pick(rng, FOCAL_SHAPES)
    dtype = pick(rng, FLOATS3)
    classes = shape[1] if len(shape) == 4 else 0
    B, H, W = shape[0], shape[-2], shape[-1]
    objs = wl.heatmap_objects(B, H, W, 0 if rng.integers(0, 4) == 0 else 1, 24, "A", seed=seed_of(rng), n_classes=classes)
    n_max = max([len(r) for r in objs[1]] + [1])
    centers, radii = np.zeros((B, n_max, 2), np.int32), np.zeros((B, n_max), np.int32)
    labels = np.zeros((B, n_max), np.int32) if classes else None
    counts = np.array([len(r) for r in objs[1]], np.int32)
    for b in range(B):
        centers[b, :counts[b]], radii[b, :counts[b]] = objs[0][b].numpy(), objs[1][b].numpy()
        if classes:
            labels[b, :counts[b]] = objs[2][b].numpy()
    hm = np.zeros(shape, np.float32)
    h1.draw_heatmap_batched(hm, centers, radii, counts, labels=labels, factor=6.0, k=1.0, clear=True)
    x = ((rng.random(shape) * 2 - 1) * 10.0)
    shift = int(rng.integers(0, 2))                       # 4 bytes: one float32 element, two 16-bit ones

    def placed(values, dt):
        lead = shift * (4 // torch.empty((), dtype=dt).element_size())
        buf = torch.zeros(values.size + lead, dtype=dt, device=device)
        buf[lead:] = torch.from_numpy(np.ascontiguousarray(values).reshape(-1)).to(dt).to(device)
        return buf[lead:].view(shape)

    kw = dict(alpha=pick(rng, [1.0, 1.5, 2.0, 3.0]), gamma=pick(rng, [0.0, 3.0, 4.0]), clamp_eps=pick(rng, [0.0, 1e-4]))
    if kw["clamp_eps"] > 0:
        # the gradient jumps to 0 where the sigmoid crosses the clamp, at |x| = log((1 - eps) / eps) = 9.2102: a float32
        # sigmoid next to 1 - 1e-4 is good to 1.2e-7, that is to 1.2e-3 in x, so within that distance a float32 evaluation
        # and the float64 definition may disagree on which side an element lies.  Logits (as rounded to the dtype: float16
        # has 9.2109 on its grid) closer than 0.01 to the edge are moved 0.02 away from it.
        edge = math.log((1 - kw["clamp_eps"]) / kw["clamp_eps"])
        xr = torch.from_numpy(x).to(dtype).double().numpy()
        a = np.abs(xr)
        x = np.where(np.abs(a - edge) < 0.01, np.sign(xr) * np.where(a >= edge, a + 0.02, a - 0.02), xr)
    if rng.integers(0, 2):
        kw.update(pos_weight=2.5, neg_weight=0.75)
    avg = pick(rng, ["default", "number", "tensor"])
    if avg != "default":
        kw["avg_factor"] = 37.5 if avg == "number" else torch.tensor(21.0, device=device)
    what = f"gaussian_focal_loss {shape} {name(dtype)} objects {counts.tolist()} {shift * 4} bytes off {kw}"
    return (placed(x, dtype), placed(hm, torch.float32)), kw, what


def gaussian_focal_definition(logits, target, alpha=2.0, gamma=4.0, pos_weight=1.0, neg_weight=1.0, clamp_eps=1e-4, avg_factor=None,
                              dtype=torch.float64, literal=True):
    """test_heatmap_loss_gpu.composition evaluated in `dtype` on the CPU (float64 and literal: the same function, checked
    by the CPU sweep); -> (loss, d loss / d logits).  literal=False takes 1 - sigmoid(x) as sigmoid(-x), as the kernel
    does (csrc/heatmap_loss.hip): the same function, without the subtraction that costs float32 its digits next to 1."""
    x = logits.detach().cpu().to(dtype).requires_grad_(True)
    t = target.detach().cpu().to(dtype)
    p = x.sigmoid()
    q = (-x).sigmoid()
    if clamp_eps > 0:
        p, q = p.clamp(clamp_eps, 1 - clamp_eps), q.clamp(clamp_eps, 1 - clamp_eps)
    pos = t.eq(1)
    # the literal spelling writes 1 - p twice, as the composition does: autograd then adds the two paths in its order
    pos_loss = -(p + 1e-12).log() * ((1 - p) if literal else q).pow(alpha) * pos
    neg_loss = -(((1 - p) if literal else q) + 1e-12).log() * p.pow(alpha) * (1 - t).pow(gamma)
    total = (pos_weight * pos_loss + neg_weight * neg_loss).sum()
    if isinstance(avg_factor, torch.Tensor):
        avg_factor = avg_factor.detach().cpu().to(dtype)
    loss = total / (pos.sum().clamp(min=1) if avg_factor is None else avg_factor)
    loss.backward()
    return loss.detach(), x.grad


def draw_center_regression(rng, device="cpu"):
    """inputs: (maps, centres [B, N, 2] int32, sizes [B], targets [B, N, C] float32, weights or None) on `device`;
    kwargs: kind, beta, avg_factor.  A third of the valid centres of every frame repeat an earlier one (duplicate cells:
    their gradients add up)."""
    import center_regression_cases as cr

    H, W = pick(rng, [1, 5, 37, 64, 260]), pick(rng, [1, 5, 37, 64, 260])
    channels = [int(c) for c in rng.integers(1, 17, size=int(rng.integers(1, 6)))]
    while sum(channels) > 64:                              # the operator's channel cap
        channels.pop()
    B = int(rng.integers(1, 7))
    while B > 1 and B * sum(channels) * H * W > 1.5e6:
        B -= 1
    while len(channels) > 1 and B * sum(channels) * H * W > 1.5e6:
        channels.pop()
    N = pick(rng, [0, 1, 63, 65, 300])
    dtype, size_dtype = pick(rng, FLOATS3), pick(rng, INTS)
    sizes = ragged_sizes(rng, B, N)
    seed = seed_of(rng)
    maps = cr.make_maps(B, channels, H, W, dtype, device, seed=seed)
    xy = cr.make_centers(B, N, H, W, sizes, "cpu", seed=seed, margin=pick(rng, [0, 2]))
    for b in range(B):
        for n in range(2, sizes[b], 3):
            xy[b, n] = xy[b, int(rng.integers(0, n))]
    C = sum(channels)
    targets = torch.from_numpy(rng.standard_normal((B, N, C)).astype(np.float32) * 3.0)
    w = pick(rng, ["none", "object", "channel"])
    if w == "none":
        # without weights every L1 (and every saturated smooth-L1) contribution to a cell is +-1 / denom: three or more of
        # them can cancel to exactly 0 in one summation order and leave a rounding residue in another, and
        # center_regression_cases.assert_grad_close wants the pattern of zeros exact.  Two cancel exactly in any order, so a
        # third centre on a cell is moved outside the map (x = -1: an invalid centre, which the operators skip).
        for b in range(B):
            seen = {}
            for n in range(sizes[b]):
                cell = (int(xy[b, n, 0]), int(xy[b, n, 1]))
                seen[cell] = seen.get(cell, 0) + 1
                if seen[cell] > 2:
                    xy[b, n, 0] = -1
    weights = None if w == "none" else torch.from_numpy(rng.random((B, N) if w == "object" else (B, N, C)).astype(np.float32))
    kw = dict(kind=pick(rng, ["l1", "smooth_l1"]), beta=pick(rng, [1.0, 1.7]))
    avg = pick(rng, ["default", "number", "tensor"])
    if avg != "default":
        kw["avg_factor"] = 37.5 if avg == "number" else torch.tensor(21.0, device=device)
    what = (f"center_regression {B} x {channels} x {H} x {W} {name(dtype)} N {N} sizes {sizes} as {name(size_dtype)} weights {w} "
            f"builder seed {seed} {kw}")
    inp = (maps, xy.to(device), torch.tensor(sizes, dtype=size_dtype, device=device), targets.to(device),
           None if weights is None else weights.to(device))
    return inp, kw, what


# ---------------------------------------------------------------------------------------------------------- error figures
def loss_error(out, want):
    """largest |out - want| / |want| over the entries whose definition is not 0"""
    o, w = out.detach().cpu().double().reshape(-1), want.detach().cpu().double().reshape(-1)
    nz = w != 0
    return float(((o - w).abs()[nz] / w.abs()[nz]).max()) if bool(nz.any()) else 0.0


def grad_error(grad, want, dtype):
    """(figure, unit): float32 / float64 gradients as the largest err / bound of the operators' mixed bound
    (1e-4 |g| + 1e-6 max|g|; float64 1e-12 / 1e-14), 16-bit ones as representable steps from the rounded float64 gradient"""
    from matched_focal_loss_cases import _ulp_steps

    g, w = grad.detach().cpu(), want.detach().cpu().double()
    if g.numel() == 0:
        return 0.0
    if dtype in (torch.float16, torch.bfloat16):
        return float(_ulp_steps(g, w.to(dtype)).max())
    rel, floor = (1e-12, 1e-14) if dtype == torch.float64 else (1e-4, 1e-6)
    bound = rel * w.abs() + floor * w.abs().max()
    ok = bound > 0
    return float(((g.double() - w).abs()[ok] / bound[ok]).max()) if bool(ok.any()) else 0.0



class Worst:
    """the largest figure seen per (operator, dtype, quantity), and the cases behind it"""

    def __init__(self):
        self.figures, self.cases = {}, {}

    def add(self, op, dtype, **figures):
        key = (op, name(dtype) if isinstance(dtype, torch.dtype) else str(dtype))
        self.cases[key] = self.cases.get(key, 0) + 1
        for q, v in figures.items():
            self.figures[key + (q,)] = max(self.figures.get(key + (q,), 0.0), float(v))

    def lines(self):
        out = []
        for key in sorted(self.cases):
            figs = ", ".join(f"{q} {v:.3e}" for (o, d, q), v in sorted(self.figures.items()) if (o, d) == key)
            out.append(f"  {key[0]} {key[1]}: {self.cases[key]} cases; {figs or 'every output bit-equal'}")
        return out


# (seed base, seeds at ACCV_FUZZ_SCALE = 1, cases per seed): shared by the CPU and the GPU sweep, which draw the same cases.
# The counts keep one seed near a second on the GPU machine, where the float64 definitions on the CPU dominate (measured:
# 0.05 .. 1.2 s per seed), and the whole CPU sweep near ten seconds.
SWEEPS = {
    "matched_focal_loss": (710000, 6, 12),
    "matched_box_loss": (720000, 6, 12),
    "batched_matching_cost": (730000, 6, 10),
    "polyline": (740000, 6, 6),
    "center_point_decode": (750000, 4, 10),
    "rotated_nms_bev": (760000, 4, 5),
    "center_point_targets": (770000, 4, 6),
    "batched_linear_sum_assignment": (780000, 6, 10),
    "heatmap_peaks": (790000, 6, 10),
    "gaussian_focal_loss": (800000, 6, 6),
    "center_regression": (810000, 6, 8),
}


def sweep(op, seed, device="cpu"):
    """yields (tag, inputs, kwargs) of the cases of one seed of an operator's sweep"""
    base, _, cases = SWEEPS[op]
    rng = np.random.default_rng(base + seed)
    draw = globals()["draw_" + op]
    for case in range(cases):
        inp, kw, what = draw(rng, device)
        yield f"seed {seed} case {case}: {what}", inp, kw
