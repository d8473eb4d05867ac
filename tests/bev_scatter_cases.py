"""Cases and the definition of scatter_to_bev, shared by test_bev_scatter_cpu.py and test_bev_scatter_gpu.py.

`definition` is the sequential loop of mmdet3d's PointPillarsScatter over the rows in order (a later row of a cell overwrites
an earlier one), in numpy on the bit patterns of the features, so that it is the same code for float32, float16 and
bfloat16; `backward_definition` hands every row that still owns its cell the gradient at that cell and +0 to all others.
Nothing is approximate: every comparison is bit for bit (NaN payloads and signed zeros count), and there is no tolerance in
this file.

The constants of the device's work partition (lanes of a workgroup, cells of a tile, channels of a chunk) are arguments,
which the GPU file reads from the source.
"""
import ctypes
import functools

import numpy as np
import torch

from accvlab.point_cloud import concatenate_voxels, scatter_to_bev, voxelize_points

import voxelize_cases as vx

DTYPES = (torch.float32, torch.float16, torch.bfloat16)
BITS = {torch.float32: torch.int32, torch.float16: torch.int16, torch.bfloat16: torch.int16}
PAYLOADS = {4: np.array([0x7FC00000, 0x7FC01234, 0xFFC00001, 0x7F800001, 0x80000000], np.uint32).view(np.int32),
            2: np.array([0x7E00, 0x7E12, 0xFE01, 0x7C01, 0x8000, 0x7FC1, 0xFFC3], np.uint16).view(np.int16)}


def bits_of(t):
    """integer view of a float tensor on the CPU"""
    t = t.detach().cpu()
    return t.view(BITS[t.dtype]) if t.dtype in BITS else t


def assert_bits(got, want, what):
    g, w = bits_of(got), (want if isinstance(want, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(want)))
    w = bits_of(w)
    assert tuple(g.shape) == tuple(w.shape), f"{what}: shape {tuple(g.shape)}, expected {tuple(w.shape)}"
    assert g.dtype == w.dtype, f"{what}: {g.dtype} for {w.dtype}"
    if not torch.equal(g, w):
        first = tuple(int(i) for i in torch.nonzero(g != w)[0])
        raise AssertionError(f"{what}: {int((g != w).sum())} elements differ, first at {first}: {int(g[first]):#x} for {int(w[first]):#x}")


# ------------------------------------------------------------------------------------------------------- the definition
def cells_of(coors, B, V, ny, nx):
    """(b, y, x) of every row and whether it is placed; coors [rows, 4] as (b, z, y, x) or [rows, 3] with b = r // V"""
    coors = np.asarray(coors, np.int64).reshape(-1, np.shape(coors)[-1])
    rows = coors.shape[0]
    b = coors[:, 0] if coors.shape[1] == 4 else np.arange(rows) // max(V, 1)
    y, x = coors[:, -2], coors[:, -1]
    return b, y, x, (b >= 0) & (b < B) & (y >= 0) & (y < ny) & (x >= 0) & (x < nx)


def definition(feature_bits, coors, B, ny, nx, V=0):
    """(canvas bits [B, C, ny, nx], index int32 [B, ny, nx]) of the sequential loop"""
    feature_bits = np.asarray(feature_bits)
    C = feature_bits.shape[-1]
    feats = feature_bits.reshape(-1, C)
    b, y, x, placed = cells_of(coors, B, V, ny, nx)
    index = np.full((B, ny, nx), -1, np.int32)
    for r in range(feats.shape[0]):
        if placed[r]:
            index[b[r], y[r], x[r]] = r          # the last row of a cell stays
    canvas = np.zeros((B, C, ny, nx), feats.dtype)
    bb, yy, xx = np.nonzero(index >= 0)
    canvas[bb, :, yy, xx] = feats[index[bb, yy, xx]]
    return canvas, index


def backward_definition(grad_bits, coors, index, B, ny, nx, V=0):
    """grad_features bits [rows, C]"""
    grad_bits, index = np.asarray(grad_bits), np.asarray(index)
    b, y, x, placed = cells_of(coors, B, V, ny, nx)
    out = np.zeros((b.shape[0], grad_bits.shape[1]), grad_bits.dtype)
    for r in range(b.shape[0]):
        if placed[r] and index[b[r], y[r], x[r]] == r:
            out[r] = grad_bits[b[r], :, y[r], x[r]]
    return out


# ----------------------------------------------------------------------------------------------------------------- cases
def random_values(seed, shape, dtype, dev):
    """normal values with NaNs of several payloads, infinities and -0.0 sprinkled in, as a tensor of `dtype`"""
    rng = np.random.default_rng(seed)
    t = torch.from_numpy(rng.standard_normal(shape).astype(np.float32)).to(dtype)
    bits = t.view(BITS[dtype]).numpy()
    hit = rng.random(shape) < 0.05
    bits[hit] = rng.choice(PAYLOADS[t.element_size()], int(hit.sum()))
    return t.to(dev)


def random_coors(seed, rows, B, ny, nx, outside=0.15):
    """int32 [rows, 4]: (b, z, y, x) with about `outside` of the rows one step outside the map or the batch, z of any sign"""
    rng = np.random.default_rng(seed)
    c = np.stack([rng.integers(0, max(B, 1), rows), rng.integers(-5, 40, rows), rng.integers(0, max(ny, 1), rows),
                  rng.integers(0, max(nx, 1), rows)], axis=1).astype(np.int32)
    out = np.flatnonzero(rng.random(rows) < outside)
    col = rng.choice(np.array([0, 2, 3]), out.size)
    side = rng.random(out.size) < 0.5
    limit = np.array([B, 0, ny, nx])[col]
    c[out, col] = np.where(side, -1, limit)
    return c


def run_case(dev, dtype, coors, B, ny, nx, C, seed, what, V=0, features=None, grad=None):
    """forward and backward of one call against the definition; returns (canvas, index, grad_features)"""
    coors = np.asarray(coors, np.int32)
    rows = int(np.prod(coors.shape[:-1]))
    lead = coors.shape[:-1]
    feats = random_values(seed, lead + (C,), dtype, dev) if features is None else features
    feats = feats.detach().requires_grad_(True)
    tc = torch.from_numpy(np.ascontiguousarray(coors)).to(dev)
    kw = dict(grid_hw=(ny, nx), return_index=True)
    if coors.shape[-1] == 4:
        kw["batch_size"] = B
    canvas, index = scatter_to_bev(feats, tc, **kw)
    assert canvas.dtype == dtype and index.dtype == torch.int32 and canvas.device.type == torch.device(dev).type
    assert tuple(canvas.shape) == (B, C, ny, nx) and tuple(index.shape) == (B, ny, nx)
    assert canvas.requires_grad and not index.requires_grad
    want_canvas, want_index = definition(bits_of(feats).numpy().reshape(rows, C), coors, B, ny, nx, V)
    assert_bits(index, want_index, f"{what}: index")
    assert_bits(canvas, want_canvas, f"{what}: canvas")
    go = random_values(seed + 1, (B, C, ny, nx), dtype, dev) if grad is None else grad
    got, = torch.autograd.grad(canvas, feats, go)
    assert got.dtype == dtype and got.shape == feats.shape
    want = backward_definition(bits_of(go).numpy(), coors, want_index, B, ny, nx, V)
    assert_bits(got.reshape(rows, C), want, f"{what}: grad_features")
    return canvas, index, got


def check_shapes(dev, dtype, nx, chunk):
    """ny in {1, 2, 5} x B in {1, 3} x C in {1, 3, 4, 8, chunk - 1, chunk, chunk + 1, 2 chunk + 3} at one nx: tile edges, rows
    that are 16-byte multiples and rows that are not, a partial last channel chunk, rows outside the map, duplicates"""
    n = 0
    for ny in (1, 2, 5):
        for B in (1, 3):
            for C in (1, 3, 4, 8, chunk - 1, chunk, chunk + 1, 2 * chunk + 3):
                rows = max(3, (B * ny * nx * 2) // 3)
                coors = random_coors(7 * nx + n, rows, B, ny, nx)
                run_case(dev, dtype, coors, B, ny, nx, C, 100 + n, f"{dtype}, B {B}, C {C}, {ny} x {nx}")
                n += 1


def check_row_counts(dev, threads):
    """0, 1, threads - 1, threads and threads + 1 rows: the edges of the mark launch's and the backward's workgroups"""
    B, ny, nx, C = 2, 9, 70, 4
    for rows in (0, 1, threads - 1, threads, threads + 1):
        for dtype in (torch.float32, torch.bfloat16):
            coors = random_coors(rows, rows, B, ny, nx, outside=0.15 if rows > 1 else 0.0)
            _, index, _ = run_case(dev, dtype, coors, B, ny, nx, C, 200 + rows, f"{rows} rows, {dtype}")
            assert rows == 0 or int((index >= 0).sum()) > 0


def check_occupancy(dev, tile):
    """a frame without any row; a tile fully occupied next to an empty one; a single occupied cell at each corner"""
    ny, nx, C = 3, 2 * tile + 2, 8
    for dtype in DTYPES:
        # frame 1 of 3 is empty, frame 0 holds the whole first tile of map row 1 and nothing else
        full = np.array([[0, 7, 1, x] for x in range(tile)] + [[2, 0, 2, nx - 1]], np.int32)
        canvas, index, _ = run_case(dev, dtype, full, 3, ny, nx, C, 300, f"full and empty tiles, {dtype}")
        assert bool((index[0, 1, :tile] >= 0).all()) and bool((index[0, 1, tile:] == -1).all()) and bool((index[1] == -1).all())
        assert not bits_of(canvas[1]).any(), "a frame without rows is not +0"
        for y, x in ((0, 0), (0, nx - 1), (ny - 1, 0), (ny - 1, nx - 1)):
            canvas, index, _ = run_case(dev, dtype, np.array([[0, 0, y, x]], np.int32), 1, ny, nx, C, 310 + x + y, f"corner {y, x}, {dtype}",
                                        features=torch.full((1, C), 2.5, dtype=dtype, device=dev))
            assert int((index >= 0).sum()) == 1 and int(index[0, y, x]) == 0
            assert int((canvas != 0).sum()) == C and bool((canvas[0, :, y, x] == 2.5).all())


def check_duplicates(dev, threads):
    """two and many rows on one cell, within a workgroup of the mark launch and across its boundaries: the highest row wins
    and the losers get a zero gradient"""
    B, ny, nx, C = 2, 4, 66, 5
    rows = 3 * threads + 7
    coors = random_coors(5, rows, B, ny, nx, outside=0.0)
    pair = [3, threads + 3]                                           # two rows, two workgroups
    many = list(range(10, rows, 37))                                  # a row of every workgroup and several of some
    near = [threads - 1, threads]                                     # neighbours across the boundary
    for group, cell in ((pair, (0, 1, 5)), (many, (1, 3, 65)), (near, (1, 0, 0))):
        coors[group, 0], coors[group, 2], coors[group, 3] = cell
    others = np.setdiff1d(np.arange(rows), pair + many + near)
    for group, cell in ((pair, (0, 1, 5)), (many, (1, 3, 65)), (near, (1, 0, 0))):     # nobody else on these cells
        hit = others[(coors[others, 0] == cell[0]) & (coors[others, 2] == cell[1]) & (coors[others, 3] == cell[2])]
        coors[hit, 3] = (coors[hit, 3] + 1) % 60 + 1
    feats = torch.arange(rows * C, dtype=torch.float32).view(rows, C).to(dev) + 1.0
    go = torch.ones((B, C, ny, nx), device=dev)
    _, index, grad = run_case(dev, torch.float32, coors, B, ny, nx, C, 0, "duplicates", features=feats, grad=go)
    for group, cell in ((pair, (0, 1, 5)), (many, (1, 3, 65)), (near, (1, 0, 0))):
        assert int(index[cell]) == max(group)
        assert bool((grad[max(group)] == 1).all()) and not grad[[g for g in group if g != max(group)]].any()
    assert len(many) > 10


def check_outside(dev):
    """each of b, y, x just outside on either side is unplaced; z of any value, negative included, has no effect"""
    B, ny, nx, C = 2, 3, 5, 4
    inside = [[1, 0, 2, 4], [0, 0, 0, 0]]
    outside = [[-1, 0, 1, 1], [B, 0, 1, 1], [0, 0, -1, 1], [0, 0, ny, 1], [0, 0, 1, -1], [0, 0, 1, nx]]
    coors = np.array(inside + outside, np.int32)
    for dtype in DTYPES:
        _, index, grad = run_case(dev, dtype, coors, B, ny, nx, C, 400, f"outside, {dtype}", features=torch.ones((8, C), dtype=dtype, device=dev),
                                  grad=torch.ones((B, C, ny, nx), dtype=dtype, device=dev))
        assert int((index >= 0).sum()) == 2 and bool((grad[:2] == 1).all()) and not grad[2:].any()
        shifted = coors.copy()
        shifted[:, 1] = [-7, 2 ** 31 - 1, 5, -2 ** 31, 0, 1, 2, 3]
        canvas_a, index_a, _ = run_case(dev, dtype, coors, B, ny, nx, C, 401, f"z, {dtype}")
        canvas_b, index_b, _ = run_case(dev, dtype, shifted, B, ny, nx, C, 401, f"other z, {dtype}")
        assert torch.equal(index_a, index_b) and torch.equal(bits_of(canvas_a), bits_of(canvas_b))


def check_padded_form(dev):
    """[B, V, C] with the coors of voxelize_points, padding included, equals the flat form on concatenate_voxels"""
    sizes = (0, 65, 700)
    pts = vx.random_points(78, sizes, 4)
    vox = voxelize_points(vx.ragged(pts, sizes, dev), max_points=3, max_voxels=90, **vx.PILLARS)
    B, V, C, ny, nx = 3, 90, 6, 16, 16
    counts = vox.voxel_counts.tolist()
    assert counts[0] == 0 and 0 < counts[1] < V and counts[2] == V and bool((vox.coors[1, counts[1]:] == -1).all())
    for dtype in DTYPES:
        feats = random_values(500, (B, V, C), dtype, dev)
        canvas, index, grad = run_case(dev, dtype, vox.coors.cpu().numpy(), B, ny, nx, C, 500, f"padded, {dtype}", V=V, features=feats)
        assert int((index >= 0).sum()) == sum(counts) and not bits_of(grad[1, counts[1]:]).any()
        _, coors4, _ = concatenate_voxels(vox)
        keep = torch.arange(V, device=dev).view(1, V) < vox.voxel_counts.view(B, 1)
        flat = feats[keep].contiguous().requires_grad_(True)
        canvas_f, index_f = scatter_to_bev(flat, coors4, grid_hw=(ny, nx), batch_size=B, return_index=True)
        assert_bits(canvas_f, canvas, f"flat against padded, {dtype}")
        assert torch.equal((index_f >= 0), (index >= 0))
        go = random_values(501, (B, C, ny, nx), dtype, dev)
        g_flat, = torch.autograd.grad(canvas_f, flat, go)
        g_pad, = torch.autograd.grad(scatter_to_bev(feats.requires_grad_(True), vox.coors, grid_hw=(ny, nx)), feats, go)
        assert_bits(g_flat, g_pad[keep], f"flat against padded gradient, {dtype}")


def off_boundary(t, elements=1):
    """a contiguous copy of `t` that starts `elements` elements behind a 16-byte boundary"""
    flat = torch.zeros(t.numel() + 8, dtype=t.dtype, device=t.device)
    view = flat[elements: elements + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == elements * t.element_size() and view.is_contiguous()
    return view


def check_misaligned(dev):
    """features and grad_canvas views off a 16-byte boundary take the element-wise path and give equal bits"""
    B, ny, nx, C = 2, 3, 72, 16
    coors = random_coors(9, 200, B, ny, nx)
    for dtype in DTYPES:
        feats = random_values(600, (200, C), dtype, dev)
        go = random_values(601, (B, C, ny, nx), dtype, dev)
        canvas, index, grad = run_case(dev, dtype, coors, B, ny, nx, C, 0, f"aligned, {dtype}", features=feats, grad=go)
        canvas_m, index_m, grad_m = run_case(dev, dtype, coors, B, ny, nx, C, 0, f"misaligned, {dtype}", features=off_boundary(feats),
                                             grad=off_boundary(go))
        for got, want, name in ((canvas_m, canvas, "canvas"), (index_m, index, "index"), (grad_m, grad, "grad_features")):
            assert_bits(got, want, f"misaligned against aligned, {name}, {dtype}")


def check_guard_bands(dev):
    """the C entries alone write all of canvas, index and grad_features and nothing outside them, 16-byte aligned (16-byte
    stores) and one element off (element-wise stores)"""
    from accvlab import _amd_native as nat

    lib = nat.ctypes_lib()
    cuda = torch.device(dev).type == "cuda"
    stream = nat.stream_ptr(torch.device(dev, torch.cuda.current_device())) if cuda else None
    sync = torch.cuda.synchronize if cuda else (lambda: None)
    B, ny, nx, C, rows, pad = 2, 3, 72, 72, 150, 512
    coors = random_coors(11, rows, B, ny, nx)
    tc = torch.from_numpy(coors).to(dev)
    for dtype in DTYPES:
        es = torch.empty((), dtype=dtype).element_size()
        for shift in (0, es):
            feats = random_values(700, (rows, C), dtype, dev)
            go = random_values(701, (B, C, ny, nx), dtype, dev)
            bufs, outs = {}, {}
            for name, shape, dt in (("canvas", (B, C, ny, nx), dtype), ("index", (B, ny, nx), torch.int32), ("grad", (rows, C), dtype)):
                nbytes = int(np.prod(shape)) * torch.empty((), dtype=dt).element_size()
                off = pad + (shift if name != "index" else 0)
                bufs[name] = torch.full((off + nbytes + pad,), 0xA5, dtype=torch.uint8, device=dev)
                outs[name] = (off, nbytes, bufs[name][off: off + nbytes].view(dt).view(shape))
            args = (feats.data_ptr(), tc.data_ptr(), rows, 0, B, C, ny, nx, 4, es, outs["canvas"][2].data_ptr(), outs["index"][2].data_ptr())
            status = lib.accv_bev_scatter(*args, stream) if cuda else lib.accv_bev_scatter_cpu(*args)
            sync()
            assert status == 0, lib.accv_last_error()
            want_canvas, want_index = definition(bits_of(feats).numpy(), coors, B, ny, nx)
            assert_bits(outs["canvas"][2].clone(), want_canvas, f"banded canvas, {dtype}, shift {shift}")
            assert_bits(outs["index"][2].clone(), want_index, f"banded index, {dtype}, shift {shift}")
            args = (go.data_ptr(), tc.data_ptr(), outs["index"][2].data_ptr(), rows, 0, B, C, ny, nx, 4, es, outs["grad"][2].data_ptr())
            status = lib.accv_bev_scatter_bwd(*args, stream) if cuda else lib.accv_bev_scatter_bwd_cpu(*args)
            sync()
            assert status == 0, lib.accv_last_error()
            assert_bits(outs["grad"][2].clone(), backward_definition(bits_of(go).numpy(), coors, want_index, B, ny, nx),
                        f"banded grad_features, {dtype}, shift {shift}")
            for name, (off, nbytes, _) in outs.items():
                assert bool((bufs[name][:off] == 0xA5).all()) and bool((bufs[name][off + nbytes:] == 0xA5).all()), f"wrote outside {name}"


def mmdet3d_scatter(features, coors, B, ny, nx):
    """mmdet3d's PointPillarsScatter.forward_batch in torch"""
    batch_canvas = []
    for b in range(B):
        canvas = torch.zeros(features.shape[1], nx * ny, dtype=features.dtype, device=features.device)
        mask = coors[:, 0] == b
        this = coors[mask, :]
        indices = (this[:, 2] * nx + this[:, 3]).long()
        canvas[:, indices] = features[mask, :].t()
        batch_canvas.append(canvas)
    return torch.stack(batch_canvas, 0).view(B, features.shape[1], ny, nx)


def check_against_torch(dev):
    """on inputs without duplicates, all placed: the forward equals mmdet3d's zeros + index assignment and the backward
    equals torch autograd through that composition (torch.equal); with duplicates torch's result is not defined"""
    B, ny, nx, C = 3, 7, 70, 10
    rng = np.random.default_rng(1)
    cells = rng.permutation(B * ny * nx)[:400]
    coors = np.stack([cells // (ny * nx), rng.integers(0, 9, 400), cells // nx % ny, cells % nx], axis=1).astype(np.int32)
    tc = torch.from_numpy(coors).to(dev)
    for dtype in DTYPES:
        feats = torch.from_numpy(rng.standard_normal((400, C)).astype(np.float32)).to(dtype).to(dev)
        go = torch.from_numpy(rng.standard_normal((B, C, ny, nx)).astype(np.float32)).to(dtype).to(dev)
        a, b = feats.clone().requires_grad_(True), feats.clone().requires_grad_(True)
        ours, theirs = scatter_to_bev(a, tc, grid_hw=(ny, nx), batch_size=B), mmdet3d_scatter(b, tc, B, ny, nx)
        assert torch.equal(ours, theirs), f"forward differs from the torch composition, {dtype}"
        ga, = torch.autograd.grad(ours, a, go)
        gb, = torch.autograd.grad(theirs, b, go)
        assert torch.equal(ga, gb), f"backward differs from torch autograd, {dtype}"


def check_empty(dev):
    """B == 0; zero rows (the canvas is still fully written); a map without cells"""
    for dtype in DTYPES:
        canvas, index = scatter_to_bev(torch.zeros((0, 5), dtype=dtype, device=dev), torch.zeros((0, 4), dtype=torch.int32, device=dev),
                                       grid_hw=(4, 6), batch_size=0, return_index=True)
        assert tuple(canvas.shape) == (0, 5, 4, 6) and tuple(index.shape) == (0, 4, 6)
        run_case(dev, dtype, np.zeros((0, 4), np.int32), 2, 3, 70, 5, 800, f"no rows, {dtype}")
        canvas, index, grad = run_case(dev, dtype, random_coors(3, 10, 2, 0, 5), 2, 0, 5, 4, 801, f"no cells, {dtype}")
        assert canvas.numel() == 0 and not bits_of(grad).any()
    padded = scatter_to_bev(torch.ones((2, 0, 3), device=dev), torch.zeros((2, 0, 3), dtype=torch.int32, device=dev), grid_hw=(2, 2))
    assert tuple(padded.shape) == (2, 3, 2, 2) and not bits_of(padded).any()


def check_errors(dev, other_dev=None):
    """every documented error is raised by the Python layer, before a launch"""
    import pytest

    feats = torch.ones((6, 4), device=dev)
    coors = torch.zeros((6, 4), dtype=torch.int32, device=dev)
    call = lambda f=feats, c=coors, **kw: scatter_to_bev(f, c, **dict(dict(grid_hw=(3, 5), batch_size=2), **kw))      # noqa: E731
    call()
    for bad in (feats.double(), feats.int()):
        with pytest.raises(TypeError, match="features"):
            call(f=bad)
    for bad in (coors.long(), coors.short(), coors.to(torch.uint8)):
        with pytest.raises(TypeError, match="coors"):
            call(c=bad)
    with pytest.raises(RuntimeError, match="coors"):
        call(c=coors.float())
    for bad in (coors[:5], coors[:, :3].contiguous(), coors.view(6, 4, 1)):
        with pytest.raises(RuntimeError, match="coors"):
            call(c=bad)
    with pytest.raises(RuntimeError, match="coors"):
        call(f=torch.ones((2, 3, 4), device=dev))
    with pytest.raises(RuntimeError, match="features"):
        call(f=torch.ones((6,), device=dev), c=coors)
    with pytest.raises(RuntimeError, match="channels"):
        scatter_to_bev(torch.ones((6, 1025), device=dev), coors, grid_hw=(3, 5), batch_size=2)
    with pytest.raises(RuntimeError, match="channels"):
        scatter_to_bev(torch.ones((6, 0), device=dev), coors, grid_hw=(3, 5), batch_size=2)
    with pytest.raises(RuntimeError, match="contiguous"):
        call(f=torch.ones((6, 8), device=dev)[:, :4])
    with pytest.raises(RuntimeError, match="contiguous"):
        call(c=torch.zeros((4, 6), dtype=torch.int32, device=dev).t())
    for bad in (None, -1, 2.0, True):
        with pytest.raises(RuntimeError, match="batch_size"):
            call(batch_size=bad)
    with pytest.raises(RuntimeError, match="batch_size"):
        scatter_to_bev(torch.ones((2, 3, 4), device=dev), torch.zeros((2, 3, 3), dtype=torch.int32, device=dev), grid_hw=(3, 5), batch_size=3)
    for bad in ((3,), (3, 5, 1), (3.0, 5), (-1, 5), 3, None):
        with pytest.raises(RuntimeError, match="grid_hw"):
            call(grid_hw=bad)
    with pytest.raises(RuntimeError, match="2\\^31"):
        call(grid_hw=(2 ** 15, 2 ** 15))
    with pytest.raises(RuntimeError, match="must be a tensor"):
        call(c=None)
    if other_dev is not None:
        with pytest.raises(RuntimeError, match="device"):
            call(c=coors.to(other_dev))
