"""From rendered depth maps to a mesh, end to end: a SHELL -- a few thousand small, opaque, flat Gaussians
on a sphere -- is rendered from 6 ring cameras and 2 polar ones at 96 x 64, the maps are fused through
``mesh.TSDFVolume`` into 40^3 samples and the zero level set is extracted.

The fusion is held to the float64 fusion of the SAME rendered maps (copied to the host) under the rule of
tests/tsdf_ref.py; the mesh to the reference extraction of the GPU's own float32 volume under the rules of
tests/test_gpu_mesh.py (counts, keys, area vectors per cell; coordinates where float32 can hold 1e-6 voxel: the lattice
has a voxel of 2^-4 and an origin that is a multiple of it).  ``Trainer.extract_mesh`` must give the manual loop's mesh
and leave parameters and optimizer state bit for bit.  The distribution of the vertex radii is printed, not asserted: how
well the expected depth sum w z / sum w of a shell of discs sits on the sphere is a property of the scene."""
import numpy as np
import pytest

from easygaussiansplatting_amd import scene as S
from tests import tsdf_ref as TR

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

N, W, H = 4000, 96, 64
DIMS, VOXEL, ORIGIN = (40, 40, 40), 0.0625, (-1.25, -1.25, -1.25)
BOUNDS = (ORIGIN, tuple(o + VOXEL * (n - 1) for o, n in zip(ORIGIN, DIMS)))


def shell_scene():
    """N discs on the unit sphere (a Fibonacci lattice): 0.045 across, 0.004 thick, opacity 0.95, coloured by position"""
    k = np.arange(N) + 0.5
    zc = np.clip(1.0 - 2.0 * k / N, -0.9995, 0.9995)
    phi = np.pi * (1.0 + 5.0 ** 0.5) * k
    r = np.sqrt(1.0 - zc * zc)
    n = np.stack([r * np.cos(phi), r * np.sin(phi), zc], 1)
    q = np.concatenate([(1.0 + n[:, 2:3]), -n[:, 1:2], n[:, 0:1], np.zeros((N, 1))], 1)       # e_z -> n
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    scales = np.tile(np.array([0.045, 0.045, 0.004]), (N, 1))
    shs = ((0.5 + 0.4 * n) - 0.5) / 0.28209479177387814
    # (a principal point off the half-pixel grid: the lattice's symmetry planes do not project onto pixel boundaries)
    cam = S.Camera(W, H, 90.0, 90.0, W / 2.0 - 0.37, H / 2.0 + 0.21, np.eye(3), np.array([0.0, 0.0, 3.5]))
    f = np.float32
    return S.Scene(n.astype(f), q.astype(f), scales.astype(f), np.full(N, 0.95, f), shs.astype(f), cam)


def cameras(base):
    cams = S.ring_cameras(base, 6, radius=3.5)
    for s in (1.0, -1.0):      # looking down and up the world y axis
        Rcw = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, s], [0.0, -s, 0.0]])
        cams.append(S.Camera(W, H, base.fx, base.fy, base.cx, base.cy, Rcw, np.array([0.0, 0.0, 3.5])))
    return cams


@pytest.fixture(scope="module")
def setup():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from easygaussiansplatting_amd import gsplatcu
    from easygaussiansplatting_amd.function import Camera, GSFunction, RenderOptions
    gsplatcu.set_policy("gsplatcu")
    sc = shell_scene()
    cams = [Camera.from_scene(c) for c in cameras(sc.cam)]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()
    maps = []
    with torch.no_grad():
        leaves = (dev(sc.pws), dev(sc.shs), dev(sc.alphas).reshape(-1, 1), dev(sc.scales), dev(sc.rots))
        for c in cams:
            image, _, depth, alpha = GSFunction.apply(*leaves, torch.zeros((N, 2), device="cuda"), c,
                                                      RenderOptions(depth=True, alpha=True))
            maps.append((image.contiguous(), depth.contiguous(), alpha.contiguous()))
    return sc, cams, maps


def host_view(cam, image, depth, alpha, trunc):
    return dict(R=cam.Rcw.cpu().numpy().astype(np.float64), t=cam.tcw.cpu().numpy().astype(np.float64),
                K=(cam.fx, cam.fy, cam.cx, cam.cy), trunc=trunc, alpha_min=0.5, near=0.01, depth_max=None,
                depth=depth[0].cpu().numpy(), alpha=alpha[0].cpu().numpy(), image=image.cpu().numpy(), weight=None)


def test_fusion_and_mesh_of_the_shell(setup):
    from easygaussiansplatting_amd.mesh import TSDFVolume
    sc, cams, maps = setup
    vol = TSDFVolume(ORIGIN, VOXEL, DIMS)
    assert vol.trunc == 4 * VOXEL
    lat = dict(dims=DIMS, origin=list(ORIGIN), voxel=VOXEL)
    s64, s32 = TR.new_state(DIMS), TR.new_state(DIMS, True, np.float32)
    dec = np.ones(DIMS[::-1], bool)
    for cam, (image, depth, alpha) in zip(cams, maps):
        assert float(alpha.max()) > 0.9 and float((alpha > 0.5).float().mean()) > 0.1
        vol.integrate(depth, alpha, cam, image=image)
        view = host_view(cam, image, depth, alpha, vol.trunc)
        dec &= TR.decided(lat, view)
        TR.integrate(s64, lat, view)
        TR.integrate(s32, lat, view, np.float32)
    torch.cuda.synchronize()
    got = dict(tsdf=vol.tsdf.cpu().numpy(), weight=vol.weight.cpu().numpy(), color=vol.color.cpu().numpy())
    seen = s64["weight"] > 0
    assert np.array_equal((got["weight"] > 0)[dec], seen[dec])
    e_ref, e_hip = TR.errors(s32, s64, dec & seen), TR.errors(got, s64, dec & seen)
    bound = TR.bounds(e_ref, s64)
    print("fusion of 8 views: %d samples seen, %d left out | e_ref %s | e_hip %s" % (
        int(seen.sum()), int((~dec).sum()), e_ref, e_hip))
    assert 1.0 - dec.mean() <= 8 * TR.UNDECIDED_CAP
    for k in e_hip:
        assert e_hip[k] <= bound[k], (k, e_hip[k], bound[k])
    assert float(s64["weight"].max()) >= 4 and (got["weight"][~seen & dec] == 0).all()

    # the mesh of the GPU's volume against the reference extraction of the same float32 planes
    verts, keys, cols = (t.cpu().numpy() for t in vol.extract_triangles())
    ref = TR.extract(lat, got["tsdf"], got["weight"], got["color"], 1.0)
    assert len(verts) == sum(len(t) for t in ref.values()) > 1000
    at, e_coord, e_area, e_col = 0, 0.0, 0.0, 0.0
    for ci in sorted(ref):
        tris = ref[ci]
        sl = slice(at, at + len(tris))
        at += len(tris)
        assert set(keys[sl].ravel().tolist()) == {k for t in tris for k in t["keys"]}, ci
        e_area = max(e_area, float(np.abs(TR.area_vector(verts[sl]) - TR.area_vector([t["v"] for t in tris])).max()))
        by_key = {t["keys"][s]: (t["v"][s], t["c"][s]) for t in tris for s in range(3)}
        for kk, vv, cc in zip(keys[sl].ravel(), verts[sl].reshape(-1, 3), cols[sl].reshape(-1, 3)):
            rv, rc = by_key[int(kk)]
            if np.abs(rv).max() < 16 * VOXEL:
                e_coord = max(e_coord, float(np.abs(vv - rv).max()))
            e_col = max(e_col, float(np.abs(cc - rc).max()))
    print("mesh: %d triangles | coordinates %.2e voxel | area vectors %.2e voxel^2 | colours %.2e" % (
        len(verts), e_coord / VOXEL, e_area / VOXEL ** 2, e_col))
    assert e_area <= 1e-5 * VOXEL ** 2 and e_coord <= 1e-6 * VOXEL and e_col <= 1e-6

    V, F, C = vol.extract()
    V, F, C = V.cpu().numpy(), F.cpu().numpy(), C.cpu().numpy()
    assert len(F) == len(verts) and len(V) == len(np.unique(keys)) and C.shape == V.shape
    assert np.isfinite(V).all() and np.isfinite(C).all()
    assert (V >= np.array(BOUNDS[0])).all() and (V <= np.array(BOUNDS[1])).all()
    assert np.array_equal(V[F], verts)                       # welding moves no vertex
    radius = np.linalg.norm(V.astype(np.float64), axis=1)
    print("vertex radii (the shell is the unit sphere): min %.3f, 5%% %.3f, median %.3f, 95%% %.3f, max %.3f; closed: %s; "
          "V - E + F = %d" % (radius.min(), *np.percentile(radius, [5, 50, 95]), radius.max(),
                              TR.closed_and_consistent(F), TR.euler(V, F)))


def test_trainer_extract_mesh_is_the_manual_loop_and_leaves_the_trainer_alone(setup):
    from easygaussiansplatting_amd.function import GSRawFunction, RenderOptions
    from easygaussiansplatting_amd.mesh import TSDFVolume
    from easygaussiansplatting_amd.trainer import Trainer
    sc, cams, maps = setup
    start = shell_scene()
    start.shs[:, :3] += 0.1
    tr = Trainer(start, cams, [m[0] for m in maps], max_steps=10, view_streams=1)
    for views in ([0, 3], [6]):
        assert np.isfinite(tr.step(views))
    snap = lambda: ({k: v.detach().clone() for k, v in tr.params.items()},
                    {k: None if v.grad is None else v.grad.detach().clone() for k, v in tr.params.items()},
                    [{n: (x.clone() if isinstance(x, torch.Tensor) else x) for n, x in st.items()}
                     for st in tr.opt.state.values()])
    before = snap()
    V, F, C = tr.extract_mesh(voxel_size=VOXEL, bounds=BOUNDS)
    after = snap()
    for a, b in zip(before[:2], after[:2]):
        for k in a:
            assert (a[k] is None and b[k] is None) or torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k
    assert len(before[2]) == len(after[2]) > 0
    for a, b in zip(before[2], after[2]):
        for n in a:
            assert torch.equal(a[n], b[n]) if isinstance(a[n], torch.Tensor) else a[n] == b[n], n
    assert not any(p.grad is not None and p.grad.requires_grad for p in tr.params.values())
    # the manual loop on the trainer's parameters
    vol = TSDFVolume(ORIGIN, VOXEL, DIMS)
    p = tr.params
    with torch.no_grad():
        for cam in cams:
            out = GSRawFunction.apply(p["pws"], p["low_shs"], p["high_shs"], p["alphas_raw"], p["scales_raw"],
                                      p["rots_raw"], torch.zeros((N, 2), device="cuda"), cam,
                                      RenderOptions(depth=True, alpha=True))
            vol.integrate(out[2], out[3], cam, image=out[0].contiguous())
    V2, F2, C2 = vol.extract()
    assert len(F) > 1000 and torch.equal(F, F2)
    assert torch.equal(V.view(torch.int32), V2.view(torch.int32)) and torch.equal(C.view(torch.int32), C2.view(torch.int32))
    # a subset of the views, the default bounds, no colour: a smaller mesh inside the scene's box
    V3, F3, C3 = tr.extract_mesh(view_ids=[0, 1], voxel_size=2 * VOXEL, color=False, alpha_min=0.6, depth_max=6.0)
    assert C3 is None and 0 < len(F3) < len(F) and bool(torch.isfinite(V3).all()) and float(V3.abs().max()) < 2.0
    with pytest.raises(ValueError, match="bounds must be"):
        tr.extract_mesh(bounds=((0, 0, 0), (1, 1, 0)))
    with pytest.raises(TypeError):
        tr.extract_mesh(view_ids=[0], no_such_option=1)
