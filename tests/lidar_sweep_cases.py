"""Seeded random draws for the sweeps of the lidar branch and the query decoders (test_lidar_sweeps_cpu.py,
test_lidar_sweeps_gpu.py), in the form of camera_sweep_cases.py (§9zb) and operator_sweep_cases.py (§9q),
whose helpers it reuses.

One function per operator: ``draw_<operator>(rng, device="cpu") -> (inputs, kwargs, description)``.  Every draw is a pure
function of the numpy generator: the seed of the generator and the number of draws taken from it reproduce a case, and
`description` names every drawn parameter for the failure message.  The inputs come from the builders of the operators' own
``*_cases.py`` modules (seeded from `rng`); what is drawn here is what those builders take as arguments.  `inputs` holds the
numpy arrays the definitions read next to the tensors on `device` that the operators read.

Every value list straddles a constant of the operator's kernel.  The constants below are literals, so that the CPU and the
GPU file draw the same cases; the GPU file reads them from the .hip sources and asserts that they are these.

All operators here but the two decoders are compared bit for bit and have no margin rule and no redraw loop.  The decoders'
only margin is the sigmoid score against `score_threshold` (see `_decoder_inputs`).
"""
import re

import numpy as np
import torch

from operator_sweep_cases import FLOATS3, INTS, Worst, name, pick, ragged_sizes, seed_of  # noqa: F401

MAX_GROUP, LDS_FLOATS = 64, 8192               # pillar_features.hip: kMaxGroup, kLdsFloats
SCAN_CHUNK = 1024 * 4                          # voxelize.hip: kScanThreads * kUnroll points of a counting workgroup
THREADS, TILE, CHUNK = 256, 64, 64             # bev_scatter.hip: kThreads, kTileW, kChunk
Q_THREADS, Q_UNROLL = 1024, 8                  # query_decode.hip: kThreads, kUnroll
# redraws of a case whose comparison sat on a threshold, per operator (the tests assert their share)
REDRAWS = {"query_box_decode_3d": 0, "query_box_decode_2d": 0}


def off_boundary(t, elements):
    """`t` itself when `elements` is 0, else a contiguous copy that starts `elements` elements behind a 16-byte boundary
    (pillar_features_cases.check_misaligned's construction, for 1..3 elements)"""
    if not elements:
        assert t.numel() == 0 or t.data_ptr() % 16 == 0
        return t
    flat = torch.zeros(t.numel() + 4, dtype=t.dtype, device=t.device)
    view = flat[elements: elements + t.numel()].view(t.shape)
    view.copy_(t)
    assert (t.numel() == 0 or view.data_ptr() % 16 == (elements * t.element_size()) % 16) and view.is_contiguous()
    return view


def _dev(device, a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(device)


# --------------------------------------------------------------------------------------- pillar_features and voxel_mean
# 33, 43 and 127 are the T at which G * T * D can be odd (G < 64 and T odd); they are listed twice so that the four
# combinations of 16-byte / 4-byte loads and stores all occur under aligned tensors at ACCV_FUZZ_SCALE = 1
PILLAR_T = [1, 2, 3, 5, 20, 32, 33, 43, 64, 127, 128, 33, 43, 127]
# voxel_size and point_cloud_range: every value exact in float32, negative and non-zero lo
PILLAR_GRIDS = [dict(voxel_size=(0.5, 0.25, 4.0), point_cloud_range=(-4.0, -2.0, -2.0, 4.0, 2.0, 2.0)),
                dict(voxel_size=(0.25, 0.5, 2.0), point_cloud_range=(-8.0, 1.0, -3.0, 8.0, 9.0, 1.0)),
                dict(voxel_size=(1.0, 0.125, 8.0), point_cloud_range=(0.0, -2.0, 0.5, 16.0, 2.0, 8.5))]


def _draw_voxels(rng, device, clean):
    """the voxels of a pillar_features / voxel_mean draw: (dict of numpy arrays, shapes and the operator's positional
    arguments on `device`, description); `clean` passes the voxels through pillar_features_cases.mean_input"""
    import pillar_features_cases as pf

    from accvlab.point_cloud import Voxels

    T, D = pick(rng, PILLAR_T), int(rng.integers(3, 17))
    G = pf.group_of(T, D, MAX_GROUP, LDS_FLOATS)
    M = pick(rng, [0, 1, G - 1, G, G + 1, 2 * G + 1, 3 * G + 2])
    cw = pick(rng, [3, 4])
    form = pick(rng, ["flat", "padded", "tuple"])
    shift = pick(rng, [0, 0, 0, 1, 2, 3])
    hostile = bool(rng.integers(0, 4) > 0)
    seed = seed_of(rng)
    vox, num, coors = pf.make_voxels(seed, M, T, D, hostile=hostile)
    if clean:
        vox = pf.mean_input(vox, num)
    coors = np.ascontiguousarray(coors[:, 4 - cw:])
    lead = (M,)
    if form != "flat":
        B = pick(rng, [b for b in (1, 2, 3) if M % b == 0])
        lead = (B, M // B)
    tv = off_boundary(_dev(device, vox), shift).view(lead + (T, D))
    tn, tc = _dev(device, num).view(lead), _dev(device, coors).view(lead + (cw,))
    assert tv.data_ptr() % 16 == 4 * shift or M == 0
    args = (Voxels(tv, tc, tn, None, None),) if form == "tuple" else (tv, tn, tc)
    inp = dict(vox=vox, num=num, coors=coors, T=T, D=D, M=M, G=G, lead=lead, shift=shift, args=args)
    what = (f"T {T} D {D} G {G} M {M} as {form} {list(lead)} coors of {cw} voxels {shift} elements off a 16-byte boundary "
            f"hostile padding {hostile} builder seed {seed}")
    return inp, what


def draw_pillar_features(rng, device="cpu"):
    """inputs: see _draw_voxels; kwargs: the operator's.  The description names the launch the device picks: `loads` and
    `stores` 16 where the base is 16-byte aligned and G * T * D (G * T * F) is a multiple of 4, else 4; the output is the
    operator's own allocation, whose alignment the check asserts"""
    import pillar_features_cases as pf

    inp, what = _draw_voxels(rng, device, clean=False)
    flags = pick(rng, pf.FLAGS)
    grid = pick(rng, PILLAR_GRIDS)
    F = pf.feature_count(inp["D"], flags)
    span = inp["G"] * inp["T"]
    vec_in, vec_out = inp["shift"] == 0 and span * inp["D"] % 4 == 0, span * F % 4 == 0
    inp["F"] = F
    what = (f"pillar_features {what} flags {flags} F {F} loads {16 if vec_in else 4} stores {16 if vec_out else 4} "
            f"bases {'aligned' if inp['shift'] == 0 else 'off'} {grid}")
    return inp, dict(pf.flag_kw(flags), **grid), what


def draw_voxel_mean(rng, device="cpu"):
    inp, what = _draw_voxels(rng, device, clean=True)
    nf = pick(rng, [None, 1, 3, inp["D"]])
    vec_in = inp["shift"] == 0 and inp["G"] * inp["T"] * inp["D"] % 4 == 0
    inp["args"] = inp["args"][:2]          # a Voxels tuple, or (voxels, num_points)
    return inp, dict(num_features=nf), f"voxel_mean {what} num_features {nf} loads {16 if vec_in else 4}"


def dispatch_of(description):
    """(loads, stores or None, bases aligned) of a pillar_features / voxel_mean description"""
    loads = int(re.search(r" loads (\d+)", description).group(1))
    stores = re.search(r" stores (\d+)", description)
    return loads, int(stores.group(1)) if stores else None, " 0 elements off a 16-byte boundary" in description


# ------------------------------------------------------------------------------------------------------- scatter_to_bev
# the multiples of 8 are listed twice: only they put 2-byte rows on the vector launch, which also wants aligned features
BEV_NX, BEV_C = [1, 3, 4, 8, 63, 64, 65, 72, 130, 8, 64, 72], [1, 3, 4, 8, 63, 64, 65, 72, 131, 8, 64, 72]


def draw_scatter_to_bev(rng, device="cpu"):
    """inputs: dict(coors numpy [rows, 4] or [B, V, 3], features and grad on `device`, each aligned or off a boundary);
    kwargs: the remaining arguments of bev_scatter_cases.run_case.  The description names the write launch the device
    picks (`vector` where features is aligned and C and nx rows are 16-byte multiples; the canvas is the operator's own
    allocation) and the number of tiles without a row in frames that have rows (the empty-tile path)"""
    import bev_scatter_cases as bs

    dtype = pick(rng, list(bs.DTYPES))
    es = torch.empty((), dtype=dtype).element_size()
    nx, ny, B, C = pick(rng, BEV_NX), pick(rng, [1, 2, 5]), int(rng.integers(1, 4)), pick(rng, BEV_C)
    cells = B * ny * nx
    rows = pick(rng, [0, 1, THREADS - 1, THREADS, THREADS + 1, max(3, 2 * cells // 3), 3 * cells])
    outside = pick(rng, [0.0, 0.15, 1.0])
    padded = bool(rng.integers(0, 2))
    shifts = pick(rng, [0, 0, 0, 1, 2, 3]), pick(rng, [0, 0, 0, 1, 2, 3])
    empty = int(rng.integers(0, B)) if rng.integers(0, 3) == 0 else None
    seed = seed_of(rng)
    V, counts = 0, None
    if padded:
        V = -(-rows // B)
        rows = B * V
        counts = ragged_sizes(rng, B, V)
        coors = bs.random_coors(seed, rows, B, ny, nx, outside)[:, 1:].reshape(B, V, 3).copy()
        for b, n in enumerate(counts):
            coors[b, n:] = -1                                    # the padding of voxelize_points
        if empty is not None:
            coors[empty] = -1
    else:
        coors = bs.random_coors(seed, rows, B, ny, nx, outside)
        if empty is not None:
            hit = coors[:, 0] == empty
            if B > 1:
                coors[hit, 0] = (empty + 1) % B
            else:
                coors[hit, 3] = nx                               # the only frame: every row outside
    b, y, x, placed = bs.cells_of(coors, B, V, ny, nx)
    occupied = np.zeros((B, ny, -(-nx // TILE)), bool)
    occupied[b[placed], y[placed], x[placed] // TILE] = True
    live = occupied.any(axis=(1, 2))
    empty_tiles = int((~occupied[live]).sum())
    feats = off_boundary(bs.random_values(seed + 1, coors.shape[:-1] + (C,), dtype, device), shifts[0])
    grad = off_boundary(bs.random_values(seed + 2, (B, C, ny, nx), dtype, device), shifts[1])
    vector = shifts[0] == 0 and (C * es) % 16 == 0 and (nx * es) % 16 == 0
    what = (f"scatter_to_bev {name(dtype)} B {B} C {C} map {ny} x {nx} rows {rows} {'padded V ' + str(V) + ' counts ' + str(counts) if padded else 'flat'} "
            f"outside {outside} frame without rows {empty} features {shifts[0]} and grad {shifts[1]} elements off a boundary "
            f"write path {'vector' if vector else 'element'} of {es} bytes, {empty_tiles} empty tiles in frames with rows, "
            f"{int(placed.sum())} rows placed on {int(occupied.sum())} tiles, builder seed {seed}")
    return dict(coors=coors, features=feats, grad=grad), dict(dtype=dtype, B=B, ny=ny, nx=nx, C=C, V=V), what


def write_path_of(description):
    """(vector path, element size, empty tiles in frames with rows) of a scatter_to_bev description"""
    m = re.search(r"write path (vector|element) of (\d) bytes, (\d+) empty tiles", description)
    return m.group(1) == "vector", int(m.group(2)), int(m.group(3))


# ------------------------------------------------------------------------------------------------------ voxelize_points
def vox_grids():
    import voxelize_cases as vx

    # WIDE65: 65 x 16 pillars, (4.125 + 4) / 0.125 = 65 exactly; every value exact in float32
    return {"PILLARS": vx.PILLARS, "VOXELS3D": vx.VOXELS3D, "FINE": vx.FINE,
            "WIDE65": dict(voxel_size=(0.125, 0.5, 4.0), point_cloud_range=(-4.0, -4.0, -2.0, 4.125, 4.0, 2.0))}


VOX_P = [1, 63, 64, 65, 255, 256, 257, 1500, SCAN_CHUNK - 1, SCAN_CHUNK + 1]


def _draw_points(rng, device, P_values, grids, D_values, T_values, V_values):
    import voxelize_cases as vx

    B, P, D = int(rng.integers(1, 4)), pick(rng, P_values), pick(rng, D_values)
    sizes = ragged_sizes(rng, B, P)
    if rng.integers(0, 2):                                       # sizes outside [0, P] are clamped
        sizes[int(rng.integers(0, B))] = P + int(rng.integers(1, 1000))
        if B > 1:
            sizes[int(rng.integers(0, B))] = -int(rng.integers(1, 1000))
    grid_name = pick(rng, grids)
    grid = vox_grids()[grid_name]
    g = vx.grid_of(**grid)[2]
    cells = int(g[0] * g[1] * g[2])
    T, V = pick(rng, T_values), pick(rng, V_values)
    if V == "above":
        V = min(P, cells) + 1                                    # above every occupied count
    aug_kind = pick(rng, ["off", "rows", "rows with an identity"])
    size_dtype, spread = pick(rng, INTS), pick(rng, [4.2, 4.5])
    seed = seed_of(rng)
    points = vx.random_points(seed, [P] * B, D, P=P, spread=spread)
    aug = None
    if aug_kind != "off":
        aug = vx.rows(seed % 100003, B)
        if aug_kind != "rows":
            aug[int(rng.integers(0, B))] = vx.IDENTITY_ROW
    inp = dict(points=points, sizes=sizes, aug=aug, ragged=vx.ragged(points, sizes, device, size_dtype),
               aug_t=None if aug is None else _dev(device, aug))
    kw = dict(max_points=T, max_voxels=V, **grid)
    what = (f"B {B} P {P} sizes {sizes} as {name(size_dtype)} D {D} grid {grid_name} max_points {T} max_voxels {V} augmentation {aug_kind} "
            f"spread {spread} builder seed {seed}")
    return inp, kw, what, (int(g[1]), int(g[0]))


def draw_voxelize_points(rng, device="cpu"):
    """inputs: dict(points, sizes, aug as numpy; the RaggedBatch and the rows on `device`); kwargs: the operator's"""
    inp, kw, what, _ = _draw_points(rng, device, VOX_P, ["PILLARS", "VOXELS3D", "FINE", "WIDE65"], [3, 4, 5, 8, 15, 16], [1, 2, 3, 10],
                                    [1, 63, 64, 65, 400, "above"])
    return inp, kw, "voxelize_points " + what


# ------------------------------------------------------------------------------------------------------ the lidar chain
def draw_lidar_chain(rng, device="cpu"):
    """voxelize_points (pillar grids) -> pillar_features on the Voxels tuple -> row 0 of every voxel as a leaf in a drawn
    dtype (the stand-in of the feature net: exact and order-free) -> scatter_to_bev on the voxels' own coors -> backward;
    and the same through concatenate_voxels and the flat forms.  inputs: as draw_voxelize_points; kwargs: `voxelize`,
    `flags`, `dtype`, `grid_hw`, `seed`"""
    import bev_scatter_cases as bs
    import pillar_features_cases as pf

    inp, kw, what, grid_hw = _draw_points(rng, device, [63, 65, 257, 1500], ["PILLARS", "FINE", "WIDE65"], [3, 4, 5, 8], [1, 3, 10],
                                          [63, 65, 400])
    flags, dtype = pick(rng, pf.FLAGS), pick(rng, list(bs.DTYPES))
    seed = seed_of(rng)
    return inp, dict(voxelize=kw, flags=flags, dtype=dtype, grid_hw=grid_hw, seed=seed), \
        f"lidar chain {what} flags {flags} features as {name(dtype)} map {grid_hw} gradient seed {seed}"


# -------------------------------------------------------------------------------------------------- lidar_depth_targets
def draw_lidar_depth_targets(rng, device="cpu"):
    """inputs: dict(case: the numpy dict of depth_targets_cases, transforms numpy or None, placed); kwargs: `size_dtype`
    and the operator's.  Oracle (b) applies to placed cases without image transforms (the module's rule)"""
    import depth_targets_cases as dt

    B, P = int(rng.integers(1, 4)), pick(rng, list(dt.RAGGED_P))
    sizes = ragged_sizes(rng, B, P)
    C, D, R = pick(rng, [1, 2, 6]), pick(rng, [3, 4, 5]), pick(rng, [3, 4])
    image_hw = pick(rng, [(32, 48), (30, 44), (17, 70)])
    downsample = pick(rng, [1, 2, 4, 16])
    bins = pick(rng, [None, dt.BINS])
    with_transforms = bool(rng.integers(0, 2))
    size_dtype = pick(rng, INTS)
    placed = bool(rng.integers(0, 2))
    seed = seed_of(rng)
    case = dt.placed_case(seed, sizes, C, D, R, image_hw, depth_bins=bins) if placed else dt.random_case(seed, sizes, C, D, R, image_hw)
    tr = dt.transforms(seed % 100003, B, C) if with_transforms else None
    kw = dict(size_dtype=size_dtype, image_hw=image_hw, downsample=downsample, depth_range=dt.DEPTH_RANGE, depth_bins=bins)
    what = (f"lidar_depth_targets B {B} P {P} sizes {sizes} as {name(size_dtype)} C {C} D {D} R {R} image {image_hw} downsample {downsample} "
            f"bins {bins} image_transforms {with_transforms} {'placed' if placed else 'random'} case builder seed {seed}")
    return dict(case=case, transforms=tr, placed=placed), kw, what


# ------------------------------------------------------------------------------------------------------ the two decoders
DECODE_N = [1, 63, 64, 65, Q_THREADS - 1, Q_THREADS, Q_THREADS + 1, Q_THREADS * Q_UNROLL - 1, Q_THREADS * Q_UNROLL, Q_THREADS * Q_UNROLL + 1]
DECODE_LIMIT = 4096        # B * Q * C at most: the cut lowers B and keeps the drawn Q * C


def _decoder_inputs(rng, op):
    """what the two decoder draws share: (B, Q, C, max_num, kind, dtypes, threshold, scores_are_logits, builder seed, logits)
    The margin rule: with logit scores and a threshold, query_decode_cases.logits has already moved every logit out of
    2 MARGIN of THR after the cast; a tensor that still holds a float64 sigmoid within MARGIN of it is built again from the
    next builder seed and counted in REDRAWS (query_decode_cases.run asserts the margin of the scores it compares)"""
    import query_decode_cases as qc

    C = pick(rng, [1, 3, 10])
    target = pick(rng, DECODE_N)
    Q = max(1, (target + int(rng.integers(0, 2)) * (C - 1)) // C)         # Q * C just below or just above the drawn edge
    B = max(1, min(int(rng.integers(1, 4)), DECODE_LIMIT // (Q * C)))
    M = pick(rng, qc.max_nums(Q * C))
    kind = pick(rng, list(qc.KINDS))
    score_dtype, row_dtype = pick(rng, FLOATS3), pick(rng, FLOATS3)
    thr = pick(rng, [None, qc.THR])
    are_logits = bool(rng.integers(0, 2))
    seed = seed_of(rng) % 1000003
    for attempt in range(10):
        cls = qc.logits(B, Q, C, kind, dtype=score_dtype, seed=seed + attempt)
        s = torch.sigmoid(cls.double())
        if not (are_logits and thr is not None) or not bool(((s - thr).abs() <= qc.MARGIN).any()):
            break
        REDRAWS[op] += 1
    else:
        raise AssertionError("ten builder seeds in a row left a score on its threshold: the draw is broken")
    kw = dict(scores_are_logits=are_logits)
    if thr is not None:
        kw["score_threshold"] = thr
    what = (f"B {B} Q {Q} C {C} (Q * C {Q * C}, drawn edge {target}) max_num {M} {kind} scores {name(score_dtype)} rows {name(row_dtype)} "
            f"builder seed {seed + attempt}")
    return B, Q, C, M, kind, row_dtype, seed + attempt, cls, kw, what


def draw_query_box_decode_3d(rng, device="cpu"):
    """inputs: (cls_scores, bbox_preds, max_num) on `device`; kwargs: the operator's"""
    import query_decode_cases as qc

    B, Q, C, M, kind, row_dtype, seed, cls, kw, what = _decoder_inputs(rng, "query_box_decode_3d")
    D, special = pick(rng, [8, 10]), bool(rng.integers(0, 2))
    if rng.integers(0, 2):
        kw["post_center_range"] = qc.RANGE
    kw["bottom_center"] = bool(rng.integers(0, 2))
    rows = qc.rows_3d(B, Q, D, dtype=row_dtype, seed=seed, special=special)
    return (cls.to(device), rows.to(device), M), kw, f"query_box_decode_3d {what} D {D} special rows {special} {kw}"


def draw_query_box_decode_2d(rng, device="cpu"):
    """inputs: (cls_scores, bbox_preds, max_num) on `device`; kwargs: the operator's, tensors on `device`"""
    import query_decode_cases as qc

    B, Q, C, M, kind, row_dtype, seed, cls, kw, what = _decoder_inputs(rng, "query_box_decode_2d")
    fmt = dict(box_format=pick(rng, ["cxcywh", "xyxy"]), normalized=bool(rng.integers(0, 2)), clip=bool(rng.integers(0, 2)),
               order_corners=bool(rng.integers(0, 2)))
    special = bool(rng.integers(0, 2))
    rows = qc.rows_2d(B, Q, fmt["box_format"], fmt["normalized"], dtype=row_dtype, seed=seed, special=special)
    per_frame, hw_dtype = bool(rng.integers(0, 2)), pick(rng, INTS)
    if per_frame:
        hw = [[int(rng.integers(0, 200)), int(rng.integers(0, 1100))] for _ in range(B)]
        hw[0] = list(qc.HW)
        kw["image_hw"] = torch.tensor(hw, dtype=hw_dtype).to(device)
    else:
        kw["image_hw"] = qc.HW
    mats = pick(rng, ["off", "regular", "one singular"])
    if mats != "off":
        kw["image_matrices"] = qc.matrices(B, seed=seed, singular=(int(rng.integers(0, B)),) if mats != "regular" else ()).to(device)
    kw.update(fmt)
    shown = {k: (v.tolist() if isinstance(v, torch.Tensor) and k == "image_hw" else v) for k, v in kw.items() if k != "image_matrices"}
    what = f"query_box_decode_2d {what} special rows {special} image_hw {'per frame ' + name(hw_dtype) if per_frame else 'common'} matrices {mats} {shown}"
    return (cls.to(device), rows.to(device), M), kw, what


# (seed base, seeds at ACCV_FUZZ_SCALE = 1, cases per seed): shared by the CPU and the GPU sweep, which draw the same cases.
# Measured seconds per seed (the slowest seed of each sweep): host entries alone in the CPU file / the GPU file on the MI355X,
# where every case runs on the device and on the host; profiles/lidar_sweeps_durations.log holds the runs.  The first test of
# a process that touches an operator also pays for its imports and the library load (0.4 to 0.7 s: scatter_to_bev's seed 0
# here, the chain's seed 0 when it runs alone).  The yardstick, in the same runs: 1.4 / 1.1 s for the slowest existing seed
# (test_nms_boxes_*sweep), so the cap of twice that is 2.8 / 2.1 s.
SWEEPS = {
    "pillar_features": (910000, 6, 24),         # 0.28 / 0.20 s
    "voxel_mean": (920000, 4, 16),              # 0.05 / 0.01 s
    "scatter_to_bev": (930000, 6, 20),          # 0.70 / 0.88 s (seed 0; the others 0.04 s)
    "voxelize_points": (940000, 4, 12),         # 0.03 / 0.03 s
    "lidar_chain": (950000, 4, 8),              # 0.06 / 0.52 s
    "lidar_depth_targets": (960000, 4, 10),     # 0.05 / 0.03 s
    "query_box_decode_3d": (970000, 4, 12),     # 0.06 / 0.02 s
    "query_box_decode_2d": (980000, 4, 12),     # 0.05 / 0.03 s
}


def sweep(op, seed, device="cpu"):
    """yields (tag, inputs, kwargs) of the cases of one seed of an operator's sweep"""
    base, _, cases = SWEEPS[op]
    rng = np.random.default_rng(base + seed)
    draw = globals()["draw_" + op]
    for case in range(cases):
        inp, kw, what = draw(rng, device)
        yield f"seed {seed} case {case}: {what}", inp, kw
