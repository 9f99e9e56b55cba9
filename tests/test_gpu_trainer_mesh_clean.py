"""``Trainer.extract_mesh`` with mesh cleaning on the shell scene of tests/test_gpu_trainer_mesh.py: with the
new arguments at their defaults it returns the bits of ``TSDFVolume.extract`` composed by hand, with them exactly
``remove_small_components`` (and ``smooth_taubin``) of that mesh; every kept face then belongs to a component that passes
the threshold; the cleaned mesh with normals survives a PLY round trip."""
import numpy as np
import pytest

from tests.test_gpu_trainer_mesh import BOUNDS, DIMS, N, ORIGIN, VOXEL, setup, shell_scene  # noqa: F401  (setup: a fixture)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

MIN_FACES = 50


def bits(t):
    return t.contiguous().view(torch.int32)


def test_extract_mesh_defaults_and_cleaning(setup, tmp_path):  # noqa: F811
    from easygaussiansplatting_amd import mesh as M
    from easygaussiansplatting_amd.function import GSRawFunction, RenderOptions
    from easygaussiansplatting_amd.trainer import Trainer
    sc, cams, maps = setup
    tr = Trainer(shell_scene(), cams, [m[0] for m in maps], max_steps=10, view_streams=1)
    out = tr.extract_mesh(voxel_size=VOXEL, bounds=BOUNDS)
    assert len(out) == 3
    V, F, C = out
    # today's result: the manual loop on the trainer's parameters
    vol = M.TSDFVolume(ORIGIN, VOXEL, DIMS)
    p = tr.params
    with torch.no_grad():
        for cam in cams:
            r = GSRawFunction.apply(p["pws"], p["low_shs"], p["high_shs"], p["alphas_raw"], p["scales_raw"], p["rots_raw"],
                                    torch.zeros((N, 2), device="cuda"), cam, RenderOptions(depth=True, alpha=True))
            vol.integrate(r[2], r[3], cam, image=r[0].contiguous())
    V0, F0, C0 = vol.extract()
    assert len(F) > 1000 and torch.equal(F, F0) and torch.equal(bits(V), bits(V0)) and torch.equal(bits(C), bits(C0))

    comp = M.connected_components(F, V.shape[0])
    sizes = comp.comp_faces[comp.comp_faces > 0].sort(descending=True).values.tolist()
    print("the shell's mesh: %d vertices, %d faces, components of %s faces" % (V.shape[0], F.shape[0], sizes[:8]))
    assert sum(sizes) == F.shape[0] and sizes[0] >= MIN_FACES

    for kw, ref in ((dict(min_component_faces=MIN_FACES), dict(min_faces=MIN_FACES)),
                    (dict(keep_largest=1), dict(keep_largest=1)),
                    (dict(min_component_faces=MIN_FACES, keep_largest=2), dict(min_faces=MIN_FACES, keep_largest=2))):
        got = tr.extract_mesh(voxel_size=VOXEL, bounds=BOUNDS, **kw)
        want = M.remove_small_components(V, F, C, **ref)
        assert len(got) == 3
        assert torch.equal(got[1], want[1]) and torch.equal(bits(got[0]), bits(want[0]))
        assert torch.equal(bits(got[2]), bits(want[2]))
        after = M.connected_components(got[1], got[0].shape[0])
        per_face = after.comp_faces[after.label[got[1][:, 0]].long()]
        assert got[1].shape[0] > 0 and int(per_face.min()) >= ref.get("min_faces", 1)
        left = after.comp_faces[after.comp_faces > 0].sort(descending=True).values.tolist()
        assert left == [s for s in sizes if s >= ref.get("min_faces", 1)][:ref.get("keep_largest", len(sizes))]
        assert int((after.comp_faces == 0).sum()) == got[0].shape[0] - len(left)       # no unreferenced vertex is left

    # smoothing on top: the same faces, the vertices of smooth_taubin
    Vs, Fs, Cs = tr.extract_mesh(voxel_size=VOXEL, bounds=BOUNDS, keep_largest=1, smooth_iterations=2)
    one = M.remove_small_components(V, F, C, keep_largest=1)
    assert torch.equal(Fs, one[1]) and torch.equal(bits(Cs), bits(one[2]))
    assert torch.equal(bits(Vs), bits(M.smooth_taubin(one[0], one[1], 2)))
    assert not torch.equal(bits(Vs), bits(one[0]))

    # the cleaned mesh with normals through a PLY file
    Vc, Fc, Cc, Nc = M.clean_mesh(V, F, C, min_faces=MIN_FACES, normals=True)
    length = Nc.double().norm(dim=1)
    assert bool(((length - 1).abs() < 1e-6).all())
    radial = Vc.double() / Vc.double().norm(dim=1, keepdim=True)
    print("normals against the radial direction: min cosine %.3f, median %.3f" % (
        float((Nc.double() * radial).sum(1).min()), float((Nc.double() * radial).sum(1).median())))
    path = str(tmp_path / "clean.ply")
    M.save_mesh_ply_with_normals(path, Vc, Fc, Cc, Nc)
    v, f, c, n = M.load_mesh_ply(path, with_normals=True)
    assert np.array_equal(v.view(np.int32), Vc.cpu().numpy().view(np.int32)) and np.array_equal(f, Fc.cpu().numpy())
    assert np.array_equal(n.view(np.int32), Nc.cpu().numpy().view(np.int32))
    assert np.abs(c - np.clip(Cc.cpu().numpy(), 0.0, 1.0)).max() <= 0.5 / 255 + 1e-6
    assert len(M.load_mesh_ply(path)) == 3
