"""``Trainer.extract_mesh`` with simplification on the shell scene of tests/test_gpu_trainer_mesh.py: with
``simplify_voxels`` = 2 it returns ``simplify_vertex_clustering`` of the plain mesh on the volume's grid -- fewer faces, none
degenerate, every vertex inside the volume --, after the cleaning when both are asked for; the plain call returns the bits it
always did."""
import pytest

from tests.test_gpu_trainer_mesh import BOUNDS, DIMS, N, ORIGIN, VOXEL, setup, shell_scene  # noqa: F401  (setup: a fixture)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


def bits(t):
    return t.contiguous().view(torch.int32)


def test_extract_mesh_with_simplification(setup):  # noqa: F811
    from easygaussiansplatting_amd import mesh as M
    from easygaussiansplatting_amd.function import GSRawFunction, RenderOptions
    from easygaussiansplatting_amd.trainer import Trainer
    sc, cams, maps = setup
    tr = Trainer(shell_scene(), cams, [m[0] for m in maps], max_steps=10, view_streams=1)
    V, F, C = tr.extract_mesh(voxel_size=VOXEL, bounds=BOUNDS)
    # the plain call: the manual loop on the trainer's parameters, bit for bit
    vol = M.TSDFVolume(ORIGIN, VOXEL, DIMS)
    p = tr.params
    with torch.no_grad():
        for cam in cams:
            r = GSRawFunction.apply(p["pws"], p["low_shs"], p["high_shs"], p["alphas_raw"], p["scales_raw"], p["rots_raw"],
                                    torch.zeros((N, 2), device="cuda"), cam, RenderOptions(depth=True, alpha=True))
            vol.integrate(r[2], r[3], cam, image=r[0].contiguous())
    V0, F0, C0 = vol.extract()
    assert len(F) > 1000 and torch.equal(F, F0) and torch.equal(bits(V), bits(V0)) and torch.equal(bits(C), bits(C0))

    lo = torch.tensor(BOUNDS[0], dtype=torch.float64, device="cuda")
    hi = torch.tensor(BOUNDS[1], dtype=torch.float64, device="cuda")
    for placement in ("quadric", "mean"):
        Vs, Fs, Cs = tr.extract_mesh(voxel_size=VOXEL, bounds=BOUNDS, simplify_voxels=2, simplify_placement=placement)
        want = M.simplify_vertex_clustering(V, F, C, cell_size=2 * VOXEL, origin=ORIGIN, placement=placement)
        assert torch.equal(Fs, want[1]) and torch.equal(bits(Vs), bits(want[0])) and torch.equal(bits(Cs), bits(want[2]))
        print("the shell's mesh, %s: %d -> %d faces, %d -> %d vertices" % (placement, F.shape[0], Fs.shape[0], V.shape[0],
                                                                           Vs.shape[0]))
        assert 0 < Fs.shape[0] < F.shape[0] and Vs.shape[0] < V.shape[0]
        a, b, c = Fs[:, 0], Fs[:, 1], Fs[:, 2]
        assert bool(((a != b) & (b != c) & (a != c)).all())                          # no degenerate face
        assert int(Fs.min()) == 0 and int(Fs.max()) == Vs.shape[0] - 1
        assert torch.unique(Fs).shape[0] == Vs.shape[0]                              # every vertex referenced
        assert torch.unique(Fs, dim=0).shape[0] == Fs.shape[0]                       # no face twice
        assert bool(torch.isfinite(Vs).all()) and bool((Vs.double() >= lo).all()) and bool((Vs.double() <= hi).all())

    # after the cleaning when both are asked for
    Vc, Fc, Cc = tr.extract_mesh(voxel_size=VOXEL, bounds=BOUNDS, keep_largest=1, smooth_iterations=2, simplify_voxels=2)
    one = M.clean_mesh(V, F, C, keep_largest=1, smooth_iterations=2)
    want = M.simplify_vertex_clustering(one[0], one[1], one[2], cell_size=2 * VOXEL, origin=ORIGIN)
    assert torch.equal(Fc, want[1]) and torch.equal(bits(Vc), bits(want[0])) and torch.equal(bits(Cc), bits(want[2]))

    with pytest.raises(ValueError, match="simplify_voxels must be a finite number > 0"):
        tr.extract_mesh(voxel_size=VOXEL, bounds=BOUNDS, simplify_voxels=0)
    # the plain call again: still the same bits
    V2, F2, C2 = tr.extract_mesh(voxel_size=VOXEL, bounds=BOUNDS)
    assert torch.equal(F2, F0) and torch.equal(bits(V2), bits(V0)) and torch.equal(bits(C2), bits(C0))
