#!/usr/bin/env python3
"""From a saved scene to a triangle mesh: render the depth map of every camera of a COLMAP model, fuse them
into a TSDF volume, write the zero level set.

    python examples/extract_mesh.py --gs data/final.npy --path /data/tandt/train [--out mesh.ply] [--voxel S]
                                    [--alpha-min 0.5] [--trunc T] [--min-weight 1] [--depth-max D] [--no-color]
                                    [--min-component-faces N] [--keep-largest K] [--smooth N] [--normals]
                                    [--simplify K] [--simplify-placement quadric|mean] [--sparse]

``--gs`` is a checkpoint of ``examples/train.py`` (.npy record array) or a 3DGS .ply; ``--path`` the dataset directory
(sparse/0/*.bin + images/) whose cameras are used.  alpha_min 0.5, a truncation of 4 voxels and min_weight 1 are
defaults nobody has tuned.  The mesh is cleaned on the GPU when asked: ``--min-component-faces`` and
``--keep-largest`` drop the floaters (connected components by face count), ``--smooth`` runs Taubin iterations (lambda 0.5,
mu -0.53: untuned as well), ``--normals`` writes area-weighted vertex normals.  ``--simplify K`` then decimates the mesh by vertex
clustering on cells of K voxels (quadric placement with an untuned regulariser of 1e-3; topology is not
preserved).  Without these flags the mesh is written as extracted.  ``--sparse`` fuses into a block-allocated volume
 that stores only the 8^3 blocks near the surfaces: ``--voxel`` may then be far finer than a dense volume could
hold; the default voxel size stays what it is.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gs", required=True, help="the saved scene (.npy record array or 3DGS .ply)")
    ap.add_argument("--path", required=True, help="dataset directory (sparse/0/*.bin + images/): the cameras")
    ap.add_argument("--out", default="mesh.ply")
    ap.add_argument("--resize", type=float, default=1.0)
    ap.add_argument("--voxel", type=float, default=None, help="voxel size in world units (default: longest side / 256)")
    ap.add_argument("--trunc", type=float, default=None, help="truncation distance (default: 4 voxels; untuned)")
    ap.add_argument("--alpha-min", type=float, default=0.5, help="opacity a pixel needs to count (untuned)")
    ap.add_argument("--min-weight", type=float, default=1.0, help="weight every corner of a meshed cell needs (untuned)")
    ap.add_argument("--depth-max", type=float, default=None, help="ignore surface farther than this from a camera")
    ap.add_argument("--no-color", action="store_true", help="a mesh without vertex colours")
    ap.add_argument("--min-component-faces", type=int, default=None, metavar="N",
                    help="drop the connected components with fewer than N faces")
    ap.add_argument("--keep-largest", type=int, default=None, metavar="K", help="keep only the K components with the most faces")
    ap.add_argument("--smooth", type=int, default=0, metavar="N", help="Taubin smoothing iterations (untuned)")
    ap.add_argument("--normals", action="store_true", help="write vertex normals (nx ny nz)")
    ap.add_argument("--simplify", type=float, default=None, metavar="K",
                    help="decimate by vertex clustering: one vertex per cell of K voxels (topology is not preserved)")
    ap.add_argument("--simplify-placement", choices=("quadric", "mean"), default="quadric",
                    help="--simplify: where a cell's vertex goes: the quadric optimum (regulariser 1e-3, untuned) or the mean")
    ap.add_argument("--sparse", action="store_true",
                    help="fuse into a block-allocated volume: only the 8^3 blocks near the surfaces are stored")
    a = ap.parse_args()

    from easygaussiansplatting_amd import scene as S
    from easygaussiansplatting_amd.dataset import GSplatDataset
    from easygaussiansplatting_amd.gau_io import load_gs
    from easygaussiansplatting_amd.mesh import save_mesh_ply_with_normals, vertex_normals
    from easygaussiansplatting_amd.trainer import Trainer

    gs = load_gs(a.gs)
    ds = GSplatDataset(a.path, resize_rate=a.resize)
    sc = S.Scene(gs["pw"].copy(), gs["rot"].copy(), gs["scale"].copy(), gs["alpha"].copy(),
                 gs["sh"].reshape(gs["sh"].shape[0], -1).copy(), None)
    tr = Trainer(sc, ds.cameras, ds.images, max_steps=1, scene_size=ds.sence_size)
    vertices, faces, colors = tr.extract_mesh(voxel_size=a.voxel, trunc=a.trunc, min_weight=a.min_weight,
                                              color=not a.no_color, min_component_faces=a.min_component_faces,
                                              keep_largest=a.keep_largest, smooth_iterations=a.smooth,
                                              simplify_voxels=a.simplify, simplify_placement=a.simplify_placement,
                                              sparse=a.sparse, alpha_min=a.alpha_min, depth_max=a.depth_max)
    normals = vertex_normals(vertices, faces, check=False) if a.normals else None
    save_mesh_ply_with_normals(a.out, vertices, faces, colors, normals)
    print("wrote %s: %d vertices, %d faces from %d views" % (a.out, vertices.shape[0], faces.shape[0], len(ds)))


if __name__ == "__main__":
    main()
