"""The lidar branch of a pillar detector (PointPillars, CenterPoint-pillar, the lidar leg of BEVFusion-style models) from the
raw points to the map its 2D backbone convolves, on the device without a host round trip, and the gradient back through it:

    voxelize_points     raw ragged points -> voxels [B, V, T, D], coors, num_points (one memset, five launches)
    pillar_features     -> the decorated rows [B, V, T, D + 6] the PFN layers read, ONE launch
    Linear + ReLU + max over T in torch (the user's PFN layers; BatchNorm left out of this example)
    scatter_to_bev      -> the dense map [B, C, ny, nx], one memset and two launches, written once, zeros included
    a loss, backward    the gradient comes back through the scatter in ONE launch

`fused_step` is that path on the padded [B, V, ...] form: no `voxel_counts` is read on the host, the padding rows of
voxelize_points (coors = -1, num_points = 0) decorate to zeros and are skipped by the scatter.  Next to it is the
mmdet3d-style torch composition it replaces: `torch_pillar_features` (PillarFeatureNet.forward up to its PFN layers),
`torch_scatter_loop` (PointPillarsScatter: a Python loop over frames) and `torch_scatter_flat` (one zeros, one index_put_).
The decoration differs from torch's in the three cluster channels only, where torch's sum has no defined order; the scatter
and its backward are compared on the same PFN weights and must give equal canvases and equal gradients.

    python3 examples/pillar_step.py [--samples 2] [--points 34000] [--channels 64]
"""
from __future__ import annotations

import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "accv-lab_amd"))   # run from a checkout
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch

from accvlab.point_cloud import concatenate_voxels, pillar_features, scatter_to_bev, voxelize_points

# 0.2 m pillars over +-51.2 m: a 512 x 512 map (nuScenes); KITTI's 0.16 m pillars: 496 x 432
NUSCENES = dict(voxel_size=(0.2, 0.2, 8.0), point_cloud_range=(-51.2, -51.2, -5.0, 51.2, 51.2, 3.0), max_points=20, max_voxels=30000)
KITTI = dict(voxel_size=(0.16, 0.16, 4.0), point_cloud_range=(0.0, -39.68, -3.0, 69.12, 39.68, 1.0), max_points=32, max_voxels=16000)
GRID_HW = {"nuscenes": (512, 512), "kitti": (496, 432)}


def grid_of(cfg):
    return dict(voxel_size=cfg["voxel_size"], point_cloud_range=cfg["point_cloud_range"])


def torch_pillar_features(features, num_points, coors, voxel_size, point_cloud_range, with_distance=False, float32_offsets=False):
    """mmdet3d's non-legacy PillarFeatureNet.forward up to its PFN layers: features [M, T, D], coors [M, 4] as (b, z, y, x).
    mmdet3d evaluates the centre offsets v / 2 + lo once in Python floats (float64) and rounds the result to float32; the
    library's definition evaluates v * 0.5f + lo in float32.  Where v and lo are not exact in float32 (0.2 and -51.2 are
    not) the two offsets can differ in their last bit, and the centre channels with them; `float32_offsets` evaluates them
    as the library does."""
    vx, vy, vz = voxel_size
    if float32_offsets:
        f = torch.tensor
        x_offset, y_offset, z_offset = (float(f(v, dtype=torch.float32) * 0.5 + f(lo, dtype=torch.float32))
                                        for v, lo in zip(voxel_size, point_cloud_range[:3]))
    else:
        x_offset, y_offset, z_offset = (v / 2 + lo for v, lo in zip(voxel_size, point_cloud_range[:3]))
    dtype = features.dtype
    features_ls = [features]
    points_mean = features[:, :, :3].sum(dim=1, keepdim=True) / num_points.type_as(features).view(-1, 1, 1)
    features_ls.append(features[:, :, :3] - points_mean)
    f_center = torch.zeros_like(features[:, :, :3])
    f_center[:, :, 0] = features[:, :, 0] - (coors[:, 3].to(dtype).unsqueeze(1) * vx + x_offset)
    f_center[:, :, 1] = features[:, :, 1] - (coors[:, 2].to(dtype).unsqueeze(1) * vy + y_offset)
    f_center[:, :, 2] = features[:, :, 2] - (coors[:, 1].to(dtype).unsqueeze(1) * vz + z_offset)
    features_ls.append(f_center)
    if with_distance:
        features_ls.append(torch.norm(features[:, :, :3], 2, 2, keepdim=True))
    out = torch.cat(features_ls, dim=-1)
    mask = torch.arange(out.shape[1], dtype=torch.int, device=out.device).view(1, -1) < num_points.int().unsqueeze(-1)
    return out * mask.unsqueeze(-1).type_as(out)


def torch_scatter_loop(features, coors, batch_size, ny, nx):
    """mmdet3d's PointPillarsScatter.forward_batch: per frame a zeros canvas, a mask, a transposed index assignment; a stack"""
    batch_canvas = []
    for b in range(batch_size):
        canvas = torch.zeros(features.shape[1], nx * ny, dtype=features.dtype, device=features.device)
        mask = coors[:, 0] == b
        this = coors[mask, :]
        indices = (this[:, 2] * nx + this[:, 3]).long()
        canvas[:, indices] = features[mask, :].t()
        batch_canvas.append(canvas)
    return torch.stack(batch_canvas, 0).view(batch_size, features.shape[1], ny, nx)


def torch_scatter_flat(features, coors, batch_size, ny, nx):
    """the same without the loop: one zeros, one flat index_put_ of all frames"""
    c = coors.long()
    canvas = torch.zeros(batch_size, ny * nx, features.shape[1], dtype=features.dtype, device=features.device)
    canvas.view(-1, features.shape[1]).index_put_(((c[:, 0] * ny + c[:, 2]) * nx + c[:, 3],), features)
    return canvas.view(batch_size, ny, nx, features.shape[1]).permute(0, 3, 1, 2).contiguous()


def pfn(decorated, weight):
    """a PFN layer without its BatchNorm: Linear, ReLU, max over the points of a pillar"""
    return torch.relu(decorated @ weight.t()).amax(dim=-2)


def fused_step(points, weight, cfg, grid_hw):
    """raw points -> canvas on the padded form: nothing here synchronises with the host"""
    vox = voxelize_points(points, **cfg)
    decorated = pillar_features(vox, **grid_of(cfg))                      # [B, V, T, D + 6]
    return scatter_to_bev(pfn(decorated, weight), vox.coors, grid_hw=grid_hw), vox


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=2)
    ap.add_argument("--points", type=int, default=34000)
    ap.add_argument("--channels", type=int, default=64)
    args = ap.parse_args()
    from voxelize_step import make_cloud

    dev = torch.device("cuda", 0) if torch.cuda.is_available() else torch.device("cpu")
    cfg, (ny, nx) = NUSCENES, GRID_HW["nuscenes"]
    B, C = args.samples, args.channels
    points = make_cloud(B, args.points, 4, dev)
    g = torch.Generator().manual_seed(2)
    w_fused = (torch.randn(C, 10, generator=g) * 0.3).to(dev).requires_grad_(True)
    w_torch = w_fused.detach().clone().requires_grad_(True)
    target = torch.randn(B, C, ny, nx, generator=g).to(dev)

    canvas, vox = fused_step(points, w_fused, cfg, (ny, nx))
    loss = (canvas - target).square().mean()
    loss.backward()

    # mmdet3d's path on the same voxels: the concatenated form (a host read of the voxel count), the torch decoration, the
    # per-frame scatter loop
    voxels, coors, num_points = concatenate_voxels(vox)
    theirs = torch_pillar_features(voxels, num_points, coors, cfg["voxel_size"], cfg["point_cloud_range"], float32_offsets=True)
    ours = pillar_features(voxels, num_points, coors, **grid_of(cfg))
    outside = [c for c in range(10) if not 4 <= c < 7]
    assert torch.equal(ours[..., outside], theirs[..., outside]), "input or centre channels differ from the torch decoration"
    double_offsets = torch_pillar_features(voxels, num_points, coors, cfg["voxel_size"], cfg["point_cloud_range"])
    last_bit = int((ours[..., 7:] != double_offsets[..., 7:]).sum())     # 0.2 and -51.2 are not exact in float32
    n = num_points.view(-1, 1, 1).double()
    live = torch.arange(voxels.shape[1], device=dev).view(1, -1, 1) < num_points.view(-1, 1, 1)
    bar = (2 * n + 2) * 2.0 ** -24 * (voxels[..., :3].abs() * live).amax(dim=1, keepdim=True).double()
    beyond = int(((ours[..., 4:7].double() - theirs[..., 4:7].double()).abs() > bar).sum())
    assert beyond == 0, f"{beyond} cluster elements beyond (2 n + 2) * 2^-24 * max |p|"
    # the scatter and its backward on the same pillar features (the padded rows, so that both sides run the same matrix
    # product; a padding row gets frame -1, which no frame of the loop selects): equal canvases, equal gradients
    V = vox.coors.shape[1]
    frame = torch.arange(B, dtype=torch.int32, device=dev).view(B, 1, 1).expand(B, V, 1)
    padded = torch.cat([torch.where(vox.coors[..., :1] >= 0, frame, -1), vox.coors], dim=2).view(B * V, 4)
    feats = pfn(pillar_features(vox, **grid_of(cfg)), w_torch).view(B * V, C)
    loop = torch_scatter_loop(feats, padded, B, ny, nx)
    assert torch.equal(canvas, loop), "canvas differs from the per-frame torch loop"
    keep = padded[:, 0] >= 0
    assert torch.equal(canvas, torch_scatter_flat(feats[keep], padded[keep], B, ny, nx)), "canvas differs from the loop-free torch composition"
    (loop - target).square().mean().backward()
    assert torch.equal(w_fused.grad, w_torch.grad), "the gradient through scatter_to_bev differs from torch autograd"
    print(f"{dev}: {vox.voxel_counts.tolist()} pillars of {points.sample_sizes.tolist()} points -> decorated {tuple(ours.shape)} -> canvas "
          f"{tuple(canvas.shape)}, loss {float(loss.detach()):.6f}")
    print(f"decoration: input and centre channels equal to torch with float32 centre offsets ({last_bit} centre elements differ from "
          f"float64 offsets rounded once), cluster elements beyond the bar: {beyond}; canvas equal to the torch loop and to the "
          f"loop-free composition; weight gradients equal: True")


if __name__ == "__main__":
    main()
