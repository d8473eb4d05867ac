"""Cases and the definition of pillar_features and voxel_mean, shared by test_pillar_features_cpu.py and
test_pillar_features_gpu.py.

`definition` and `mean_definition` restate the docstring of accvlab.point_cloud.pillar_features in numpy float32, operation
by operation (numpy rounds every float32 operation once and contracts nothing): the sequential sum over the rows in row order
starting from row 0 itself, one division, one subtraction, the centre as float(c) * v + (v * 0.5 + lo), the distance as
sqrt((x * x + y * y) + z * z).  Nothing in the operators is approximate: every comparison is bit for bit, floats as int32
views, so that NaN payloads and the sign of zero count.  The only tolerances in this file are those of the comparison with
the torch composition of mmdet3d's forward: in its three cluster channels, whose sum order torch does not define, and in
the distance channel, where torch.norm's operation order is as undefined (check_against_torch writes both bars out).  The
mean over a channel that holds a NaN is a NaN whose payload is the processor's choice; the mean cases keep away from it.

The constants of the device's work partition (the most voxels a workgroup takes and its LDS budget in floats) are arguments,
which the GPU file reads from the source.
"""
import ctypes
import itertools

import numpy as np
import torch

from accvlab.batching_helpers import RaggedBatch
from accvlab.point_cloud import Voxels, concatenate_voxels, pillar_features, voxel_mean, voxelize_points

import voxelize_cases as vx

f32 = np.float32
GRID = dict(voxel_size=(0.5, 0.25, 4.0), point_cloud_range=(-4.0, -2.0, -2.0, 4.0, 2.0, 2.0))     # exact in float32 and float64
FLAGS = list(itertools.product((False, True), repeat=3))      # (cluster, centre, distance)
HOSTILE = np.array([0x7FC00000, 0xFFC00001, 0x7F800000, 0xFF800000, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F800001], np.uint32)
PAYLOADS = np.array([0x7FC00000, 0x7FC01234, 0xFFC00001, 0x7F800001, 0x80000000], np.uint32)


def bits_of(t):
    return vx.bits_of(t)


def assert_bits(got, want, what):
    g, w = bits_of(got), bits_of(want)
    assert got.dtype == torch.float32, f"{what}: {got.dtype}"
    assert tuple(g.shape) == tuple(w.shape), f"{what}: shape {tuple(g.shape)}, expected {tuple(w.shape)}"
    if not torch.equal(g, w):
        first = tuple(int(i) for i in torch.nonzero(g != w)[0])
        raise AssertionError(f"{what}: {int((g != w).sum())} elements differ, first at {first}: {int(g[first]):#x} for {int(w[first]):#x}")


# ------------------------------------------------------------------------------------------------------- the definition
def _means(vox, n, channels):
    """s_k / float(n) over the rows j < n in row order, [M, channels]; +0.0 where n == 0"""
    M, T, _ = vox.shape
    with np.errstate(all="ignore"):
        s = vox[:, 0, :channels].copy()
        for j in range(1, T):
            s = np.where((j < n)[:, None], s + vox[:, j, :channels], s)
        mean = s / n.astype(f32)[:, None]
    return np.where((n > 0)[:, None], mean, f32(0.0)).astype(f32)


def definition(voxels, num_points, coors, *, voxel_size, point_cloud_range, with_cluster_center=True, with_voxel_center=True,
               with_distance=False):
    voxels = np.asarray(voxels, f32)
    lead, (T, D) = voxels.shape[:-2], voxels.shape[-2:]
    vox = voxels.reshape(-1, T, D)
    n = np.clip(np.asarray(num_points, np.int64).reshape(-1), 0, T)
    coors = np.asarray(coors, np.int32)
    c = coors.reshape(vox.shape[0], coors.shape[-1])[:, [-1, -2, -3]]
    v, lo = np.asarray(voxel_size, f32), np.asarray(point_cloud_range[:3], f32)
    live = np.arange(T)[None, :] < n[:, None]
    parts = [np.where(live[:, :, None], vox.view(np.uint32), np.uint32(0)).view(f32)]
    with np.errstate(all="ignore"):
        xyz = vox[:, :, :3]
        if with_cluster_center:
            parts.append(xyz - _means(vox, n, 3)[:, None, :])
        if with_voxel_center:
            centre = c.astype(f32) * v + (v * f32(0.5) + lo)
            parts.append(xyz - centre[:, None, :])
        if with_distance:
            parts.append(np.sqrt((xyz[:, :, 0] * xyz[:, :, 0] + xyz[:, :, 1] * xyz[:, :, 1]) + xyz[:, :, 2] * xyz[:, :, 2])[:, :, None])
    out = np.concatenate([parts[0]] + [np.where(live[:, :, None], p, f32(0.0)).astype(f32) for p in parts[1:]], axis=2)
    return out.reshape(lead + (T, out.shape[-1]))


def mean_definition(voxels, num_points, num_features=None):
    voxels = np.asarray(voxels, f32)
    lead, (T, D) = voxels.shape[:-2], voxels.shape[-2:]
    nf = D if num_features is None else num_features
    n = np.clip(np.asarray(num_points, np.int64).reshape(-1), 0, T)
    return _means(voxels.reshape(-1, T, D), n, nf).reshape(lead + (nf,))


# ----------------------------------------------------------------------------------------------------------------- cases
def group_of(T, D, max_group, lds_floats):
    """the voxels a workgroup takes: check this against the source where the constants are read from it"""
    return max(1, min(max_group, lds_floats // (T * D)))


def make_voxels(seed, M, T, D, hostile=True, payloads=True):
    """(voxels [M, T, D], num_points [M], coors [M, 4]): point counts cycle through 0, 1, 2, T - 1, T, above T and negative;
    rows j < n are finite in x, y, z and carry NaNs of several payloads in their other channels; rows j >= n, and all rows of
    an empty voxel, hold NaN, infinities and the largest finite values when `hostile`, else +0.0; some coors are -1"""
    rng = np.random.default_rng(seed)
    vox = rng.uniform(-4.0, 4.0, (M, T, D)).astype(f32)
    counts = np.array([0, 1, 2, T - 1, T, T + 7, -3, T // 2], np.int64)
    num = counts[rng.permutation(M) % counts.size] if M else np.zeros((0,), np.int64)
    if D > 3 and M and payloads:
        extra = vox[:, :, 3:].view(np.uint32)
        hit = rng.random(extra.shape) < 0.15
        extra[hit] = rng.choice(PAYLOADS, int(hit.sum()))
        vox[:, :, 3:] = extra.view(f32)
    dead = np.arange(T)[None, :] >= np.clip(num, 0, T)[:, None]
    fill = rng.choice(HOSTILE, (M, T, D)).view(f32) if hostile else np.zeros((M, T, D), f32)
    vox = np.where(dead[:, :, None], fill, vox).astype(f32)
    coors = rng.integers(0, 16, (M, 4)).astype(np.int32)
    if M:
        coors[rng.random(M) < 0.2] = -1
        coors[np.flatnonzero(num > 0)[:1]] = -1       # at least one voxel with points has them
    return vox, num.astype(np.int32), coors


def mean_input(vox, num):
    """`vox` with the NaNs of its live rows replaced by 1.5: a mean over a NaN is a NaN whose payload is the processor's
    choice, which no definition fixes; the hostile padding stays"""
    live = np.arange(vox.shape[1])[None, :] < np.clip(num, 0, vox.shape[1])[:, None]
    return np.where(live[:, :, None] & np.isnan(vox), f32(1.5), vox).astype(f32)


def to_dev(dev, *arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays)


def flag_kw(flags):
    return dict(with_cluster_center=flags[0], with_voxel_center=flags[1], with_distance=flags[2])


# ---------------------------------------------------------------------------------------- the checks both test files run
def check_shapes(dev, T, max_group, lds_floats):
    """D in {3, 4, 5, 8, 15, 16} x M in {0, 1, G - 1, G, G + 1, 2 G + 1}: every flag subset and num_features in {1, 3, D} at
    2 G + 1 voxels, a rotating subset at the others; every point count of make_voxels, hostile padding, coors of -1"""
    turn = 0
    for D in (3, 4, 5, 8, 15, 16):
        G = group_of(T, D, max_group, lds_floats)
        for M in sorted({0, 1, G - 1, G, G + 1, 2 * G + 1}):
            vox, num, coors = make_voxels(1000 * T + 10 * D + M % 7, M, T, D)
            tv, tn, tc = to_dev(dev, vox, num, coors)
            subsets = FLAGS if M == 2 * G + 1 else [FLAGS[turn % 8]]
            turn += 1
            for flags in subsets:
                got = pillar_features(tv, tn, tc, **flag_kw(flags), **GRID)
                assert got.device.type == torch.device(dev).type and not got.requires_grad
                assert_bits(got, definition(vox, num, coors, **flag_kw(flags), **GRID), f"T {T}, D {D}, M {M}, flags {flags}")
            clean = mean_input(vox, num)
            tm, = to_dev(dev, clean)
            for nf in sorted({1, 3, D}) if M == 2 * G + 1 else (None,):
                assert_bits(voxel_mean(tm, tn, num_features=nf), mean_definition(clean, num, nf), f"mean: T {T}, D {D}, M {M}, nf {nf}")
            if M == 2 * G + 1:      # the case is what its comment says
                n = np.clip(num, 0, T)
                assert {0, 1, min(2, T), T - 1, T} <= set(n.tolist()) and (num > T).any() and (num < 0).any()
                assert ((coors == -1).all(1) & (n > 0)).any(), "no voxel with points has coors of -1"
                out = definition(vox, num, coors, **GRID)
                assert np.isfinite(out).sum() > 0 and not np.isnan(out[..., :3]).any() and not np.isnan(out[..., D:]).any(), \
                    "hostile padding reached the definition's output"
                if D > 3:
                    stored = out[..., 3:D].view(np.uint32)
                    assert (stored == 0x7FC01234).any() and (stored == 0x7F800001).any(), "no NaN payload rides in a live row"


def check_forms(dev):
    """[B, V, T, D] gives the bits of its flattened call; a Voxels tuple stands for the three tensors; coors of 3 and of 4
    columns read the same three"""
    B, V, T, D = 3, 37, 5, 4
    vox, num, coors = make_voxels(5, B * V, T, D)
    tv, tn, tc = to_dev(dev, vox, num, coors)
    flat = pillar_features(tv, tn, tc, with_distance=True, **GRID)
    assert tuple(flat.shape) == (B * V, T, D + 7)
    padded = pillar_features(tv.view(B, V, T, D), tn.view(B, V), tc[:, 1:].contiguous().view(B, V, 3), with_distance=True, **GRID)
    assert tuple(padded.shape) == (B, V, T, D + 7)
    assert_bits(padded.view(B * V, T, D + 7), flat, "padded form")
    tup = Voxels(tv.view(B, V, T, D), tc[:, 1:].contiguous().view(B, V, 3), tn.view(B, V), None, None)
    assert_bits(pillar_features(tup, with_distance=True, **GRID), padded, "Voxels tuple")
    assert_bits(voxel_mean(tup), voxel_mean(tv, tn).view(B, V, D), "Voxels tuple, mean")
    assert tuple(voxel_mean(tup, num_features=3).shape) == (B, V, 3)
    before = [t.clone() for t in (tv, tn, tc)]
    pillar_features(tv, tn, tc, **GRID)
    for now, then in zip((tv, tn, tc), before):
        assert torch.equal(bits_of(now), bits_of(then)), "an input was modified"


def check_after_voxelize(dev):
    """the real output of voxelize_points on a small ragged batch, padded and concatenated, against the definition"""
    sizes = (0, 65, 700)
    pts = vx.random_points(77, sizes, 5)
    vox = voxelize_points(vx.ragged(pts, sizes, dev), max_points=6, max_voxels=90, **vx.PILLARS)
    counts = vox.voxel_counts.tolist()
    assert counts[0] == 0 and 0 < counts[1] < 90 and counts[2] == 90
    kw = dict(with_distance=True, **vx.PILLARS)
    got = pillar_features(vox, **kw)
    want = definition(vox.voxels.cpu().numpy(), vox.num_points.cpu().numpy(), vox.coors.cpu().numpy(), **kw)
    assert_bits(got, want, "padded output of voxelize_points")
    assert not bits_of(got[0]).any(), "a frame without points is not all +0.0"
    fv, fc, fn = concatenate_voxels(vox)
    got_flat = pillar_features(fv, fn, fc, **kw)
    assert_bits(got_flat, definition(fv.cpu().numpy(), fn.cpu().numpy(), fc.cpu().numpy(), **kw), "concatenated output of voxelize_points")
    assert_bits(got_flat, torch.cat([got[b, :n] for b, n in enumerate(counts)]), "concatenated against padded")
    clean = mean_input(vox.voxels.cpu().numpy().reshape(-1, 6, 5), vox.num_points.cpu().numpy().reshape(-1))
    assert_bits(voxel_mean(torch.from_numpy(clean).to(dev), vox.num_points.view(-1)), mean_definition(clean, vox.num_points.cpu().numpy().reshape(-1)),
                "mean after voxelize")


def check_misaligned(dev):
    """a voxels view one element off a 16-byte boundary: 4-byte loads, the same bits"""
    for T, D in ((20, 4), (3, 8)):
        vox, num, coors = make_voxels(9, 131, T, D, payloads=False)
        flat = torch.zeros(vox.size + 1, dtype=torch.float32, device=dev)
        view = flat[1:].view(vox.shape)
        view.copy_(torch.from_numpy(vox))
        assert view.data_ptr() % 16 == 4 and view.is_contiguous()
        _, tn, tc = to_dev(dev, vox, num, coors)
        assert_bits(pillar_features(view, tn, tc, **GRID), definition(vox, num, coors, **GRID), f"misaligned, T {T}, D {D}")
        assert_bits(voxel_mean(view, tn), mean_definition(vox, num), f"misaligned mean, T {T}, D {D}")


def check_guard_bands(dev, max_group, lds_floats):
    """the C entries alone write all of their output and nothing outside it: with a 16-byte aligned output (16-byte stores
    where the workgroup's range allows) and with one 4 bytes off (4-byte stores)"""
    from accvlab import _amd_native as nat

    lib = nat.ctypes_lib()
    cuda = torch.device(dev).type == "cuda"
    stream = nat.stream_ptr(torch.device(dev, torch.cuda.current_device())) if cuda else None
    pad = 512
    for (T, D), shift in itertools.product(((20, 4), (7, 5), (128, 16)), (0, 4)):
        M = 2 * group_of(T, D, max_group, lds_floats) + 1
        vox, num, coors = make_voxels(21 + T, M, T, D, payloads=False)
        tv, tn, tc = to_dev(dev, vox, num, coors)
        p = nat.PillarFeaturesParams()
        p.voxels, p.num_points, p.coors = tv.data_ptr(), tn.data_ptr(), tc.data_ptr()
        p.voxel_size[:], p.range_min[:] = GRID["voxel_size"], GRID["point_cloud_range"][:3]
        p.coor_width, p.flags = 4, nat.PF_CLUSTER | nat.PF_CENTER
        for name, shape in (("features", (M, T, D + 6)), ("mean", (M, D))):
            nbytes = 4 * int(np.prod(shape))
            buf = torch.full((pad + shift + nbytes + pad,), 0xA5, dtype=torch.uint8, device=dev)
            out = buf[pad + shift: pad + shift + nbytes].view(torch.float32).view(shape)
            assert out.data_ptr() % 16 == shift
            if name == "features":
                args = (ctypes.addressof(p), M, T, D, out.data_ptr())
                status = lib.accv_pillar_features(*args, stream) if cuda else lib.accv_pillar_features_cpu(*args)
                want = definition(vox, num, coors, **GRID)
            else:
                args = (tv.data_ptr(), tn.data_ptr(), M, T, D, D, out.data_ptr())
                status = lib.accv_voxel_mean(*args, stream) if cuda else lib.accv_voxel_mean_cpu(*args)
                want = mean_definition(vox, num)
            if cuda:
                torch.cuda.synchronize()
            assert status == 0, lib.accv_last_error()
            assert bool((buf[:pad + shift] == 0xA5).all()) and bool((buf[pad + shift + nbytes:] == 0xA5).all()), f"wrote outside {name}"
            assert_bits(out.clone(), want, f"banded {name}, T {T}, D {D}, shift {shift}")


# (T, D, flags, G * T * D % 4 == 0, G * T * F % 4 == 0) with G from the device's constants (64, 8192): the smallest shapes at
# which a workgroup's own range, not a base address, is the reason for 4-byte loads, 4-byte stores, or either alone
DISPATCH = [(43, 3, (False, False, False), False, False),       # G 63, F 3: G T D = G T F = 8127
            (43, 3, (False, False, True), False, True),         # G 63, F 4: loads 4-byte, stores 16-byte
            (43, 4, (True, False, False), True, False)]         # G 47, F 7: G T D = 8084, G T F = 14147
DISPATCH_MEAN = (43, 3, (1, 3))


def feature_count(D, flags):
    return D + 3 * flags[0] + 3 * flags[1] + flags[2]


def check_dispatch(dev, max_group, lds_floats):
    """both tensors 16-byte aligned and G * T * D or G * T * F no multiple of 4: from the second workgroup on the range of
    a workgroup starts off a 16-byte boundary, which is what sends the launch to its 4-byte loads or stores (all three
    mixed instantiations of the decoration, and the 4-byte voxel mean on an aligned input).  Through the operators at
    M in {G - 1, G, G + 1, 2 G + 1} against the definition (and the host entry when `dev` is a GPU), then through the C
    entries alone into guard-banded, 16-byte aligned outputs: the 4-byte store path has no vector tail to hide an overrun"""
    from accvlab import _amd_native as nat

    lib = nat.ctypes_lib()
    cuda = torch.device(dev).type == "cuda"
    stream = nat.stream_ptr(torch.device(dev, torch.cuda.current_device())) if cuda else None
    pad = 512

    def banded(shape):
        nbytes = 4 * int(np.prod(shape))
        buf = torch.full((pad + nbytes + pad,), 0xA5, dtype=torch.uint8, device=dev)
        out = buf[pad: pad + nbytes].view(torch.float32).view(shape)
        assert out.data_ptr() % 16 == 0, "the banded output is not 16-byte aligned"
        return buf, out, nbytes

    def intact(buf, nbytes):
        if cuda:
            torch.cuda.synchronize()
        return bool((buf[:pad] == 0xA5).all()) and bool((buf[pad + nbytes:] == 0xA5).all())

    for T, D, flags, in_by_4, out_by_4 in DISPATCH:
        G, F = group_of(T, D, max_group, lds_floats), feature_count(D, flags)
        assert ((G * T * D) % 4 == 0, (G * T * F) % 4 == 0) == (in_by_4, out_by_4), f"T {T}, D {D}, {flags}: G {G} is not the regime"
        counts = sorted({G - 1, G, G + 1, 2 * G + 1})
        assert counts[-2] > G, "no workgroup with a base off a 16-byte boundary"
        for M in counts:
            what = f"dispatch T {T}, D {D}, flags {flags}, M {M}"
            vox, num, coors = make_voxels(3000 + 10 * D + M % 7, M, T, D)
            tv, tn, tc = to_dev(dev, vox, num, coors)
            assert tv.data_ptr() % 16 == 0, f"{what}: voxels are not 16-byte aligned"
            got = pillar_features(tv, tn, tc, **flag_kw(flags), **GRID)
            assert got.data_ptr() % 16 == 0 and tuple(got.shape) == (M, T, F), f"{what}: the output is not 16-byte aligned"
            want = definition(vox, num, coors, **flag_kw(flags), **GRID)
            assert_bits(got, want, what)
            if cuda:
                assert_bits(got, pillar_features(*to_dev("cpu", vox, num, coors), **flag_kw(flags), **GRID), what + ", host entry")
            p = nat.PillarFeaturesParams()
            p.voxels, p.num_points, p.coors = tv.data_ptr(), tn.data_ptr(), tc.data_ptr()
            p.voxel_size[:], p.range_min[:] = GRID["voxel_size"], GRID["point_cloud_range"][:3]
            p.coor_width = 4
            p.flags = (nat.PF_CLUSTER if flags[0] else 0) | (nat.PF_CENTER if flags[1] else 0) | (nat.PF_DISTANCE if flags[2] else 0)
            buf, out, nbytes = banded((M, T, F))
            args = (ctypes.addressof(p), M, T, D, out.data_ptr())
            status = lib.accv_pillar_features(*args, stream) if cuda else lib.accv_pillar_features_cpu(*args)
            assert status == 0, lib.accv_last_error()
            assert intact(buf, nbytes), f"{what}: wrote outside features"
            assert_bits(out.clone(), want, what + ", banded")

    T, D, widths = DISPATCH_MEAN
    G = group_of(T, D, max_group, lds_floats)
    assert (G * T * D) % 4 != 0
    for M in sorted({G - 1, G, G + 1, 2 * G + 1}):
        vox, num, _ = make_voxels(3100 + M % 7, M, T, D)
        clean = mean_input(vox, num)
        tm, tn = to_dev(dev, clean, num)
        assert tm.data_ptr() % 16 == 0
        for nf in widths:
            what = f"dispatch mean T {T}, D {D}, M {M}, nf {nf}"
            got, want = voxel_mean(tm, tn, num_features=nf), mean_definition(clean, num, nf)
            assert got.data_ptr() % 16 == 0
            assert_bits(got, want, what)
            if cuda:
                assert_bits(got, voxel_mean(*to_dev("cpu", clean, num), num_features=nf), what + ", host entry")
            buf, out, nbytes = banded((M, nf))
            args = (tm.data_ptr(), tn.data_ptr(), M, T, D, nf, out.data_ptr())
            status = lib.accv_voxel_mean(*args, stream) if cuda else lib.accv_voxel_mean_cpu(*args)
            assert status == 0, lib.accv_last_error()
            assert intact(buf, nbytes), f"{what}: wrote outside mean"
            assert_bits(out.clone(), want, what + ", banded")


def mmdet3d_forward(features, num_points, coors, voxel_size, point_cloud_range, with_distance):
    """mmdet3d's non-legacy PillarFeatureNet.forward up to its PFN layers, in torch"""
    vx_, vy, vz = voxel_size
    x_offset, y_offset, z_offset = (v / 2 + lo for v, lo in zip(voxel_size, point_cloud_range[:3]))
    dtype = features.dtype
    features_ls = [features]
    points_mean = features[:, :, :3].sum(dim=1, keepdim=True) / num_points.type_as(features).view(-1, 1, 1)
    features_ls.append(features[:, :, :3] - points_mean)
    f_center = torch.zeros_like(features[:, :, :3])
    f_center[:, :, 0] = features[:, :, 0] - (coors[:, 3].to(dtype).unsqueeze(1) * vx_ + x_offset)
    f_center[:, :, 1] = features[:, :, 1] - (coors[:, 2].to(dtype).unsqueeze(1) * vy + y_offset)
    f_center[:, :, 2] = features[:, :, 2] - (coors[:, 1].to(dtype).unsqueeze(1) * vz + z_offset)
    features_ls.append(f_center)
    if with_distance:
        features_ls.append(torch.norm(features[:, :, :3], 2, 2, keepdim=True))
    out = torch.cat(features_ls, dim=-1)
    T = out.shape[1]
    mask = (torch.arange(T, dtype=torch.int, device=out.device).view(1, -1) < num_points.int().unsqueeze(-1)).unsqueeze(-1).type_as(out)
    return out * mask


def live_rows(num, T):
    return (torch.arange(T, device=num.device).view(1, T) < num.view(-1, 1)).double()


def check_against_torch(dev):
    """torch's composition of mmdet3d's forward on clean voxels (+0.0 padding, every voxel holds a point, finite channels):
    only the three cluster channels may differ, by at most (2 n + 2) * 2^-24 * max_j |p_jk| (two summation orders of n
    terms, one division, one subtraction); the input and centre channels are torch.equal.  mmdet3d's default is
    with_distance=False; with it on, the distance channel is held to the bar written out below.

    That bar is a relaxation of "every other channel is torch.equal", and the only one: equality with torch.norm cannot
    hold together with the definition sqrt((x * x + y * y) + z * z).  Measured with these cases: on the host 145 of 2100
    (T 7) and 327 of 6000 (T 20) elements of torch.norm differ from the definition, on the MI355X 164 and 349, and on the
    host torch.norm equals none of the float32 orders of the three squares nor their float64 sum rounded once.  The largest
    difference seen is 0.41 of the bar."""
    for T, D, dist in ((20, 4, False), (32, 5, False), (7, 3, True), (20, 4, True)):
        rng = np.random.default_rng(T)
        M = 300
        vox = rng.uniform(-4.0, 4.0, (M, T, D)).astype(f32)
        num = rng.integers(1, T + 1, M).astype(np.int32)
        vox[np.arange(T)[None, :] >= num[:, None]] = 0.0
        coors = rng.integers(0, 16, (M, 4)).astype(np.int32)
        tv, tn, tc = to_dev(dev, vox, num, coors)
        got = pillar_features(tv, tn, tc, with_distance=dist, **GRID)
        ref = mmdet3d_forward(tv, tn, tc, GRID["voxel_size"], GRID["point_cloud_range"], dist)
        assert got.shape == ref.shape
        keep = [c for c in range(D + 6) if not D <= c < D + 3]
        worst = [(c, int((got[..., c] != ref[..., c]).sum())) for c in keep if not torch.equal(got[..., c], ref[..., c])]
        if dist:
            # torch.norm's operation order is as undefined as its sum's (on the host it equals none of the float32 orders of
            # x * x, y * y, z * z), so this channel has a bar as well: each evaluation is within 2.5 * 2^-24 of the exact
            # norm (three roundings in the sum of squares, halved by the root, and the root's own half), two of them differ
            # by at most 5 * 2^-24 * |p|
            norm = tv[..., :3].double().square().sum(-1).sqrt() * live_rows(tn, T)
            d_err = (got[..., D + 6].double() - ref[..., D + 6].double()).abs()
            d_over = int((d_err > 5.0 * 2.0 ** -24 * norm).sum())
            print(f"  distance channel: {int((got[..., D + 6] != ref[..., D + 6]).sum())} elements differ from torch.norm, "
                  f"max error / bound {float((d_err / (5.0 * 2.0 ** -24 * norm).clamp_min(1e-300)).max()):.3f}, beyond the bar: {d_over}")
            assert d_over == 0, f"T {T}, D {D}: {d_over} distance elements beyond 5 * 2^-24 * |p|"
        print(f"pillar_features vs torch, T {T}, D {D}: channels that differ outside the cluster group: {worst}")
        live = torch.arange(T, device=tv.device).view(1, T) < tn.view(M, 1)
        big = (tv[..., :3].abs() * live.unsqueeze(-1)).amax(dim=1, keepdim=True)                       # max_j |p_jk|
        bound = (2.0 * tn.double().view(M, 1, 1) + 2.0) * 2.0 ** -24 * big.double()
        err = (got[..., D:D + 3].double() - ref[..., D:D + 3].double()).abs()
        over = int((err > bound).sum())
        print(f"  cluster channels: max error / bound {float((err / bound.clamp_min(1e-300)).max()):.3f}, beyond the bar: {over}")
        assert not worst, f"T {T}, D {D}: channels outside the cluster group differ from torch: {worst}"
        assert over == 0, f"T {T}, D {D}: {over} cluster elements beyond (2 n + 2) * 2^-24 * max |p|"


def check_errors(dev, other_dev=None):
    """every documented error is raised by the Python layer, before a launch"""
    import pytest

    vox, num, coors = make_voxels(3, 10, 4, 5)
    tv, tn, tc = to_dev(dev, vox, num, coors)
    call = lambda v=tv, n=tn, c=tc, **kw: pillar_features(v, n, c, **dict(GRID, **kw))      # noqa: E731
    call()
    with pytest.raises(TypeError, match="float32"):
        call(v=tv.double())
    with pytest.raises(TypeError, match="float32"):
        voxel_mean(tv.half(), tn)
    for bad in (torch.zeros((10, 4, 2), device=dev), torch.zeros((10, 4, 17), device=dev), torch.zeros((10, 129, 4), device=dev),
                torch.zeros((10, 0, 4), device=dev), torch.zeros((10, 4), device=dev), torch.zeros((10, 4, 5), dtype=torch.int32, device=dev)):
        with pytest.raises(RuntimeError, match="voxels"):
            call(v=bad)
        with pytest.raises(RuntimeError, match="voxels"):
            voxel_mean(bad, tn)
    with pytest.raises(RuntimeError, match="contiguous"):
        call(v=torch.zeros((10, 4, 10), device=dev)[:, :, :5])
    with pytest.raises(RuntimeError, match="contiguous"):
        call(c=torch.zeros((4, 10), dtype=torch.int32, device=dev).t())
    for bad in (tn.long(), tn[:9], tn.view(10, 1), tn.float()):
        with pytest.raises(RuntimeError, match="num_points"):
            call(n=bad)
        with pytest.raises(RuntimeError, match="num_points"):
            voxel_mean(tv, bad)
    for bad in (tc.long(), tc[:9], tc[:, :2].contiguous(), torch.zeros((10, 5), dtype=torch.int32, device=dev),
                torch.zeros((10, 1, 4), dtype=torch.int32, device=dev)):
        with pytest.raises(RuntimeError, match="coors"):
            call(c=bad)
    with pytest.raises(RuntimeError, match="must be a tensor"):
        call(c=None)
    with pytest.raises(RuntimeError, match="Voxels"):
        pillar_features(Voxels(tv, tc, tn, None, None), tn, **GRID)
    for bad in ((0.5, 0.5), (0.5, 0.0, 4.0), (0.5, -0.5, 4.0), (0.5, float("nan"), 4.0), (0.5, float("inf"), 4.0), (1e-60, 0.5, 4.0),
                (0.5, 0.5, "4"), 0.5):
        with pytest.raises(RuntimeError, match="voxel_size"):
            call(voxel_size=bad)
    for bad in ((-4.0, -4.0, -2.0), (float("nan"), -4.0, -2.0, 4.0, 4.0, 2.0), (-4.0, float("-inf"), -2.0, 4.0, 4.0, 2.0),
                (-4.0, -4.0, 1e60, 4.0, 4.0, 2.0), (-4.0, -4.0, None, 4.0, 4.0, 2.0)):
        with pytest.raises(RuntimeError, match="point_cloud_range"):
            call(point_cloud_range=bad)
    with pytest.raises(RuntimeError, match="with_distance"):
        call(with_distance=1)
    for bad in (0, 6, 3.0, True):
        with pytest.raises(RuntimeError, match="num_features"):
            voxel_mean(tv, tn, num_features=bad)
    if other_dev is not None:
        with pytest.raises(RuntimeError, match="device"):
            call(n=tn.to(other_dev))
        with pytest.raises(RuntimeError, match="device"):
            call(c=tc.to(other_dev))
        with pytest.raises(RuntimeError, match="device"):
            voxel_mean(tv, tn.to(other_dev))


def check_empty(dev):
    tv = torch.zeros((0, 5, 4), device=dev)
    tn, tc = torch.zeros((0,), dtype=torch.int32, device=dev), torch.zeros((0, 4), dtype=torch.int32, device=dev)
    assert tuple(pillar_features(tv, tn, tc, **GRID).shape) == (0, 5, 10)
    assert tuple(voxel_mean(tv, tn).shape) == (0, 4)
    assert tuple(pillar_features(tv.view(2, 0, 5, 4), tn.view(2, 0), tc[:, 1:].reshape(2, 0, 3), **GRID).shape) == (2, 0, 5, 10)
