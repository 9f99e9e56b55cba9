"""``Trainer.save_compressed`` on the small synthetic scene the other trainer tests use: every attribute of
what ``load_compressed`` reads back is within the codec's derived bounds of what ``Trainer.save`` writes, the SH rest of every
Gaussian is the float16 rounding of the centroid it was assigned, ``weight_by="max"`` gives another codebook, and the file
is smaller than the ``.npy``."""
import json
import os

import numpy as np
import pytest

from easygaussiansplatting_amd import scene as S
from tests import kmeans_ref as KR

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

N, W, H = 2000, 128, 96


@pytest.fixture(scope="module")
def trainer():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from easygaussiansplatting_amd import gsplatcu
    from easygaussiansplatting_amd.function import Camera, render
    from easygaussiansplatting_amd.trainer import Trainer
    gsplatcu.set_policy("gsplatcu")
    sc = S.small_scene(N, W, H, 48)
    cams = [Camera.from_scene(c) for c in S.ring_cameras(sc.cam, 3, radius=5.0)]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()
    with torch.no_grad():
        gts = [render(dev(sc.pws), dev(sc.shs), dev(sc.alphas), dev(sc.scales), dev(sc.rots), c)[0].contiguous() for c in cams]
    return Trainer(S.small_scene(N, W, H, 48), cams, gts, max_steps=10, view_streams=1)


def test_save_compressed_round_trip(trainer, tmp_path):
    from easygaussiansplatting_amd import compress as CP
    from easygaussiansplatting_amd import gau_io
    npy, gsz = str(tmp_path / "s.npy"), str(tmp_path / "s.gsz")
    gs = trainer.save(npy)
    d = trainer.save_compressed(gsz, clusters=300, iters=4)
    out = CP.load_compressed(gsz)
    assert out.dtype == gs.dtype and out.shape == gs.shape == (N,)
    assert out.tobytes() == gau_io.load_gs(gsz).tobytes()
    meta = json.loads(d["meta"])
    assert meta["n"] == N and meta["sh_dim"] == 48 and meta["clusters"] == 300 and meta["bits"] == CP.DEFAULT_BITS
    f8 = lambda a: np.asarray(a, np.float64)
    assert (np.abs(f8(out["pw"]) - f8(gs["pw"])) <= KR.column_bound(d["pw_min"], d["pw_max"], 16)).all()
    log_scale = CP._dequantise(d["scale"], d["scale_min"], d["scale_max"], 8)                # the field the decoder exponentiates
    assert (np.abs(f8(log_scale) - np.log(f8(gs["scale"]))) <= KR.column_bound(d["scale_min"], d["scale_max"], 8)).all()
    assert (np.abs(np.log(f8(out["scale"])) - np.log(f8(gs["scale"]))) <= KR.column_bound(d["scale_min"], d["scale_max"], 8)).all()
    assert (np.abs(f8(out["sh"][:, :3]) - f8(gs["sh"][:, :3])) <= KR.column_bound(d["sh_dc_min"], d["sh_dc_max"], 8)).all()
    assert np.abs(f8(out["alpha"]) - f8(gs["alpha"])).max() <= 1.0 / 510
    q, q0 = f8(out["rot"]), f8(gs["rot"])
    q0 = q0 / np.linalg.norm(q0, axis=1, keepdims=True)
    assert np.abs(np.linalg.norm(q, axis=1) - 1).max() <= 1e-6
    chord = np.minimum(np.linalg.norm(q - q0, axis=1), np.linalg.norm(q + q0, axis=1))
    assert (4 * np.arcsin(chord / 2)).max() <= KR.quaternion_angle_bound(8)
    # the SH rest: the float16 rounding of the centroid each Gaussian was assigned; the index is the nearest centroid of the
    # float32 codebook k-means returned, which the archive holds only rounded -- so check against a fresh run
    rest = torch.from_numpy(np.ascontiguousarray(gs["sh"][:, 3:])).cuda()
    c, labels = CP.kmeans(rest, 300, iters=4)
    assert np.array_equal(d["sh_rest_index"], labels.cpu().numpy().astype(np.uint16))
    assert d["sh_rest_codebook"].tobytes() == c.cpu().numpy().astype(np.float16).tobytes()
    assert np.array_equal(out["sh"][:, 3:], d["sh_rest_codebook"].astype(np.float32)[d["sh_rest_index"]])
    gap = KR.gaps(gs["sh"][:, 3:], c.cpu().numpy(), labels.cpu().numpy())
    assert (gap <= KR.gap_bound(gs["sh"][:, 3:], c.cpu().numpy())).all()
    print("%d B -> %d B" % (os.path.getsize(npy), os.path.getsize(gsz)))
    assert os.path.getsize(gsz) < os.path.getsize(npy)


def test_weight_by_importance(trainer, tmp_path):
    from easygaussiansplatting_amd import compress as CP
    plain = trainer.save_compressed(str(tmp_path / "a.gsz"), clusters=100, iters=3)
    for weight_by in ("max", "sum"):
        d = trainer.save_compressed(str(tmp_path / "w.gsz"), clusters=100, iters=3, weight_by=weight_by)
        assert d["sh_rest_codebook"].shape == (100, 45) and np.isfinite(d["sh_rest_codebook"].astype(np.float32)).all()
        assert d["sh_rest_codebook"].tobytes() != plain["sh_rest_codebook"].tobytes()
        assert CP.load_compressed(str(tmp_path / "w.gsz")).shape == (N,)
    st = trainer.importance()
    rest = np.ascontiguousarray(trainer.save(str(tmp_path / "s.npy"))["sh"][:, 3:])
    c, _ = CP.kmeans(torch.from_numpy(rest).cuda(), 100, iters=3, weights=st.max.contiguous())
    d = trainer.save_compressed(str(tmp_path / "w.gsz"), clusters=100, iters=3, weight_by="max")
    assert d["sh_rest_codebook"].tobytes() == c.cpu().numpy().astype(np.float16).tobytes()
    with pytest.raises(ValueError, match="weight_by"):
        trainer.save_compressed(str(tmp_path / "w.gsz"), weight_by="hits")
