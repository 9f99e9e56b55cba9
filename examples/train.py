#!/usr/bin/env python3
"""Counterpart of the reference's ``train.py`` on the MI355X path.

    python examples/train.py --path /data/tandt/train [--epochs 100] [--resize 1.0]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 \\
        examples/train.py --path /data/tandt/train            # one camera view per GPU and step

Same schedule as train.py:44-83 -- shuffled views, densification every 5th and alpha reset every 15th
epoch in (1, 50], a checkpoint every 10th epoch and ``final.npy`` in the reference's record layout -- on
``GSplatDataset`` (COLMAP model + images), ``Trainer`` (fused render / loss / Adam kernels, RCCL
all-reduce of the gradients when launched with several ranks).  No matplotlib preview.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--path", required=True, help="dataset directory (sparse/0/*.bin + images/)")
    ap.add_argument("--epochs", type=int, default=100)
    ap.add_argument("--resize", type=float, default=1.0)
    ap.add_argument("--out", default="data")
    ap.add_argument("--antialiased", action="store_true",
                    help="anti-aliased rendering: opacity compensation of the 2D filter (DESIGN §3.9)")
    ap.add_argument("--absgrad", action="store_true",
                    help="densify on the absolute screen-space gradient (AbsGS, DESIGN §3.10); the statistic is larger "
                         "than the signed one: set --grad-threshold with it")
    ap.add_argument("--grad-threshold", type=float, default=None,
                    help="densification threshold on the accumulated screen-space gradient norm (default: 4e-7)")
    ap.add_argument("--pose-opt", action="store_true",
                    help="also refine the camera poses (a twist per camera, per-row Adam; DESIGN §3.8); the refined "
                         "poses go to poses.npz.  The default rates come from frozen-map refinement on a synthetic "
                         "scene and are not tuned for joint training")
    ap.add_argument("--pose-lr-rot", type=float, default=2e-3, help="pose Adam step of the rotation, radians")
    ap.add_argument("--pose-lr-trans", type=float, default=4e-3,
                    help="pose Adam step of the translation, as a fraction of the camera distance")
    ap.add_argument("--strategy", choices=("default", "mcmc"), default="default",
                    help="densification: the reference's clone / split / prune / alpha reset, or MCMC relocation with "
                         "a hard cap on the number of Gaussians (DESIGN §3.11; needs --cap-max)")
    ap.add_argument("--cap-max", type=int, default=None, help="--strategy mcmc: the largest number of Gaussians")
    ap.add_argument("--sparse-adam", action="store_true",
                    help="visibility-masked Adam (DESIGN §3.14): a Gaussian no view of the step saw keeps its parameters "
                         "and moments; not with --strategy mcmc")
    ap.add_argument("--bilagrid", action="store_true",
                    help="per-image appearance compensation (DESIGN §3.15): a bilateral grid of affine colour transforms "
                         "per training image absorbs exposure, white balance and vignetting; the grids are saved as "
                         "grids.npz")
    ap.add_argument("--bilagrid-shape", type=int, nargs=3, default=(16, 16, 8), metavar=("GW", "GH", "L"),
                    help="--bilagrid: nodes of a grid along x, y and luminance (1 1 1 = exposure / white balance only)")
    ap.add_argument("--masks", action="store_true",
                    help="per-pixel loss weights (DESIGN §3.16): masks/<image file name>.png (COLMAP's convention, 0 = "
                         "ignore), masks/<stem>.png or the image's alpha channel; an image without one counts every pixel")
    ap.add_argument("--depths", action="store_true",
                    help="depth supervision (DESIGN §3.17): depths/<stem>.npy (float32 disparity, 0 = no data) or "
                         "depths/<stem>.png (16-bit, value / 65536); sparse/0/depth_params.json makes the priors metric")
    ap.add_argument("--depth-kind", choices=("metric", "affine", "pearson"), default=None,
                    help="--depths: the loss (default: metric with depth_params.json, else affine: scale and shift fitted "
                         "per view and step)")
    ap.add_argument("--depth-weight", type=float, nargs=2, default=(1.0, 0.01), metavar=("INIT", "FINAL"),
                    help="--depths: the weight of the depth term decays exponentially from INIT to FINAL (the official "
                         "code's values; not tuned here)")
    ap.add_argument("--normals", action="store_true",
                    help="surface-normal supervision (DESIGN §3.18): normals/<stem>.npy ([H,W,3] or [3,H,W], camera frame, "
                         "all zero = no data) or normals/<stem>.png (8-bit RGB, n = rgb / 127.5 - 1)")
    ap.add_argument("--normals-convention", choices=("opencv", "opengl"), default="opencv",
                    help="--normals: the frame of the files: opencv (x right, y down, z forward) or opengl (y up, z "
                         "towards the viewer)")
    ap.add_argument("--normal-weight", type=float, default=0.05, metavar="W",
                    help="--normals: the weight of the prior term (not tuned here)")
    ap.add_argument("--normal-smooth", type=float, default=0.0, metavar="S",
                    help="the weight of the edge-aware smoothness of the rendered depth's normal, for every view; needs "
                         "no prior (0: off; not tuned here)")
    ap.add_argument("--prune-importance-at", default="", metavar="E[,E...]",
                    help="epochs at whose end Gaussians are pruned on their blending weight over all training views "
                         "(DESIGN §3.12); needs --prune-threshold or --prune-fraction")
    ap.add_argument("--prune-score", choices=("max", "sum", "hits"), default="max",
                    help="the statistic pruned on: largest weight (RadSplat), summed weight (Mini-Splatting), pixels hit")
    ap.add_argument("--prune-threshold", type=float, default=None, help="keep Gaussians whose score is at least this")
    ap.add_argument("--prune-fraction", type=float, default=None, help="drop this share of the Gaussians, lowest score first")
    ap.add_argument("--mesh", default=None, metavar="OUT.ply",
                    help="after training, fuse the depth maps of all training views into a TSDF volume and write its "
                         "zero level set as a triangle mesh (Trainer.extract_mesh, DESIGN §3.19; alpha_min 0.5, "
                         "truncation 4 voxels, min_weight 1: untuned defaults)")
    ap.add_argument("--mesh-voxel", type=float, default=None, metavar="S",
                    help="--mesh: the voxel size in world units (default: the longest side of the scene's box / 256)")
    ap.add_argument("--mesh-min-faces", type=int, default=None, metavar="N",
                    help="--mesh: drop the connected components (floaters) with fewer than N faces (DESIGN §3.20)")
    ap.add_argument("--mesh-simplify", type=float, default=None, metavar="K",
                    help="--mesh: decimate by vertex clustering, one vertex per cell of K voxels (DESIGN §3.21; quadric "
                         "placement, regulariser untuned; topology is not preserved)")
    ap.add_argument("--mesh-sparse", action="store_true",
                    help="--mesh: fuse into a block-allocated volume (DESIGN §3.22) that stores only the 8^3 blocks near "
                         "the surfaces, so that --mesh-voxel may be far finer than a dense volume could hold")
    ap.add_argument("--save-compressed", default=None, metavar="OUT.gsz",
                    help="after training, also write the scene compressed (DESIGN §3.23): SH rest against a k-means "
                         "codebook, other attributes at 8 or 16 bits (the number of centroids is gsplat's default, untuned)")
    a = ap.parse_args()
    if a.strategy == "mcmc" and a.cap_max is None:
        ap.error("--strategy mcmc needs --cap-max")
    if a.sparse_adam and a.strategy == "mcmc":
        ap.error("--sparse-adam is not supported with --strategy mcmc")
    if a.depths and a.absgrad:
        ap.error("--depths is not supported with --absgrad")
    if (a.normals or a.normal_smooth > 0) and a.absgrad:
        ap.error("--normals / --normal-smooth are not supported with --absgrad")
    prune_at = sorted({int(e) for e in a.prune_importance_at.split(",") if e.strip()})
    if prune_at and (a.prune_threshold is None) == (a.prune_fraction is None):
        ap.error("--prune-importance-at needs exactly one of --prune-threshold / --prune-fraction")

    import torch
    import torch.distributed as dist
    from easygaussiansplatting_amd import scene as S
    from easygaussiansplatting_amd.dataset import GSplatDataset
    from easygaussiansplatting_amd.trainer import Trainer

    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local_rank)
    if world > 1:
        dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
    rank = dist.get_rank() if world > 1 else 0
    print("Try to training %s ..." % a.path) if rank == 0 else None
    ds = GSplatDataset(a.path, resize_rate=a.resize, masks=a.masks, depths=a.depths, normals=a.normals,
                       normals_convention=a.normals_convention)
    gs = ds.gs
    start = S.Scene(gs["pw"].copy(), gs["rot"].copy(), gs["scale"].copy(), gs["alpha"].copy(), gs["sh"].copy(),
                    None)
    views_per_step = world
    steps = (len(ds) // views_per_step) * a.epochs
    tr = Trainer(start, ds.cameras, ds.images, max_steps=steps, scene_size=ds.sence_size, antialiased=a.antialiased,
                 absgrad=a.absgrad, grad_threshold=a.grad_threshold, pose_opt=a.pose_opt,
                 pose_lr=(a.pose_lr_rot, a.pose_lr_trans), strategy=a.strategy, cap_max=a.cap_max,
                 sparse_adam=a.sparse_adam, bilagrid=a.bilagrid, bilagrid_shape=tuple(a.bilagrid_shape),
                 pixel_weights=ds.weights, depth_priors=ds.depth_priors,
                 depth_kind=a.depth_kind or ds.depth_kind or "affine", depth_weight=tuple(a.depth_weight),
                 normal_priors=ds.normal_priors, normal_weight=a.normal_weight, normal_smooth=a.normal_smooth)
    os.makedirs(a.out, exist_ok=True)
    for epoch in range(a.epochs):
        loss = tr.fit(1, views_per_step=views_per_step, rng_seed=epoch, densify_until=-1)[0]
        if rank == 0:
            print("epoch:%d avg_loss:%f gaussians:%d" % (epoch, loss, tr.params["pws"].shape[0]))
        if 1 < epoch <= 50:                                   # train.py:70-76
            if epoch % 5 == 0:
                tr.densify(verbose=rank == 0)
            if epoch % 15 == 0 and a.strategy == "default":     # (MCMC relocates dead Gaussians instead)
                tr.reset_alpha()
        if epoch in prune_at:
            tr.prune_by_importance(a.prune_score, a.prune_threshold, a.prune_fraction, verbose=rank == 0)
        if epoch % 10 == 0 and rank == 0:
            tr.save(os.path.join(a.out, "epoch%04d.npy" % epoch))
    if rank == 0:
        tr.save(os.path.join(a.out, "final.npy"))
        if a.pose_opt:
            tr.save_poses(os.path.join(a.out, "poses.npz"))
        if a.bilagrid:
            tr.save_grids(os.path.join(a.out, "grids.npz"))
        if a.save_compressed:
            tr.save_compressed(a.save_compressed)
            print("compressed scene: %d B -> %s" % (os.path.getsize(a.save_compressed), a.save_compressed))
        print("Training is finished.")
        if a.mesh:
            from easygaussiansplatting_amd.mesh import save_mesh_ply
            vertices, faces, colors = tr.extract_mesh(voxel_size=a.mesh_voxel, min_component_faces=a.mesh_min_faces,
                                                      simplify_voxels=a.mesh_simplify, sparse=a.mesh_sparse)
            save_mesh_ply(a.mesh, vertices, faces, colors)
            print("mesh: %d vertices, %d faces -> %s" % (vertices.shape[0], faces.shape[0], a.mesh))
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
