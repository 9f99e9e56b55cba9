"""COLMAP scene as a training set: the counterpart of ``gsplat/gausplat_dataset.py``.

``GSplatDataset(path)`` expects ``path/sparse/0/{cameras,images,points3D}.bin`` and ``path/images/*``;
item ``i`` is ``(Camera, image[3,H,W] float32 in [0,1] on the device)``; ``.gs`` holds the initial
Gaussians (cached as ``points3D.npy`` next to the model, like the reference) and ``.sence_size``
(sic) = 1.1 x the largest camera-centre distance from the mean centre (gausplat_dataset.py:67-69).
PIL decodes the images (the reference goes through torchvision's ``to_tensor``: uint8 HWC -> float
CHW / 255).

``GSplatDataset(path, masks=True)`` also collects a per-pixel loss weight per image (``.weights[i]``: float32 [H,W] in
[0,1] on the device, or None), for ``Trainer(pixel_weights=ds.weights)``.  Looked for in this order:
``path/masks/<image file name>.png`` (COLMAP's convention: ``images/a.jpg`` -> ``masks/a.jpg.png``, 0 = ignore),
``path/masks/<stem>.png``, the image's own alpha channel.  The mask is read as 8-bit grey, resized with the image and
scaled by 1/255.

``GSplatDataset(path, depths=True)`` also collects a depth prior per image (``.depth_priors[i]``: float32 [H,W]
DISPARITY -- inverse depth, 0 = no data -- on the device, or None) and ``.depth_kind``, for
``Trainer(depth_priors=ds.depth_priors, depth_kind=ds.depth_kind)``.  Looked for in this order:
``path/depths/<stem>.npy`` (float32 disparity), ``path/depths/<stem>.png`` (16-bit grey, value / 65536: the convention of
the official code's monocular depth maps).  A prior is resized with the image by NEAREST sampling, so that a no-data
pixel never bleeds into its neighbours.  With ``path/sparse/0/depth_params.json`` (the official
``{image stem: {"scale": s, "offset": o}}``) every prior becomes s q + o where it has data and ``depth_kind`` is
"metric"; otherwise ``depth_kind`` is "affine" (scale and shift are fitted during training).

``GSplatDataset(path, normals=True)`` also collects a normal prior per image (``.normal_priors[i]``: float32 [3,H,W]
CAMERA-frame unit normals -- x right, y down, z forward; all zero = no data -- on the device, or None), for
``Trainer(normal_priors=ds.normal_priors)``.  Looked for in this order: ``path/normals/<stem>.npy``
(float, [H,W,3] or [3,H,W]), ``path/normals/<stem>.png`` (8-bit RGB, n = rgb / 127.5 - 1).  ``normals_convention``:
"opencv" (the frame above, the default) or "opengl" (y up, z towards the viewer: y and z are flipped on reading).
Resized with the image by NEAREST sampling.
"""
from __future__ import annotations

import json
import os

import numpy as np
import torch

from . import colmap
from .function import Camera as RenderCamera


class Camera(RenderCamera):
    """Render camera + the bookkeeping fields of gausplat_dataset.py:14-26."""

    def __init__(self, id, width, height, fx, fy, cx, cy, Rcw, tcw, path=None, device="cuda"):
        super().__init__(width, height, fx, fy, cx, cy, Rcw, tcw, device=device, id=id, path=path)


def _to_tensor(img, device):
    a = np.array(img.convert("RGB"), dtype=np.uint8)   # (a writable copy: torch.from_numpy warns otherwise)
    return torch.from_numpy(a).to(device).permute(2, 0, 1).to(torch.float32).div_(255.0).contiguous()


def _weight_source(path, name, image):
    """The image's mask as a PIL "L" image, or None: masks/<name>.png, masks/<stem>.png, the alpha channel."""
    from PIL import Image
    for cand in (name + ".png", os.path.splitext(name)[0] + ".png"):
        fn = os.path.join(path, "masks", cand)
        if os.path.exists(fn):
            return Image.open(fn).convert("L")
    if "A" in image.getbands():
        return image.getchannel("A")
    return None


def _nearest(a, width, height):
    """``a`` [h,w] sampled to [height,width] at the nearest source pixel (pixel centres; no value is blended)"""
    h, w = a.shape
    if (h, w) == (height, width):
        return a
    rows = np.minimum(((np.arange(height) + 0.5) * h / height).astype(np.int64), h - 1)
    cols = np.minimum(((np.arange(width) + 0.5) * w / width).astype(np.int64), w - 1)
    return a[rows[:, None], cols[None, :]]


def _depth_source(path, name):
    """The image's depth prior as a float32 [h,w] disparity array, or None: depths/<stem>.npy, depths/<stem>.png."""
    stem = os.path.splitext(name)[0]
    fn = os.path.join(path, "depths", stem + ".npy")
    if os.path.exists(fn):
        a = np.load(fn)
        if a.ndim != 2:
            raise ValueError("%s: expected a [H,W] disparity array, got shape %s" % (fn, list(a.shape)))
        return a.astype(np.float32)
    fn = os.path.join(path, "depths", stem + ".png")
    if os.path.exists(fn):
        from PIL import Image
        im = Image.open(fn)
        if im.mode not in ("I;16", "I;16B", "I;16L", "I"):
            raise ValueError("%s: expected a 16-bit grey image, got mode %s" % (fn, im.mode))
        return (np.asarray(im).astype(np.float64) / 65536.0).astype(np.float32)
    return None


NORMALS_CONVENTIONS = ("opencv", "opengl")


def _normal_source(path, name):
    """The image's normal prior as a float32 [3,h,w] array, or None: normals/<stem>.npy, normals/<stem>.png."""
    stem = os.path.splitext(name)[0]
    fn = os.path.join(path, "normals", stem + ".npy")
    if os.path.exists(fn):
        a = np.load(fn)
        if a.ndim == 3 and a.shape[2] == 3:      # ([H,W,3]; a [3,H,3] array is read as this form too)
            a = a.transpose(2, 0, 1)
        elif a.ndim != 3 or a.shape[0] != 3:
            raise ValueError("%s: expected a [H,W,3] or [3,H,W] array of normals, got shape %s" % (fn, list(a.shape)))
        return a.astype(np.float32)
    fn = os.path.join(path, "normals", stem + ".png")
    if os.path.exists(fn):
        from PIL import Image
        im = Image.open(fn)
        if im.mode not in ("RGB", "RGBA"):
            raise ValueError("%s: expected an 8-bit RGB image, got mode %s" % (fn, im.mode))
        rgb = np.asarray(im.convert("RGB"), dtype=np.uint8)
        return (rgb.astype(np.float32) / np.float32(127.5) - np.float32(1)).transpose(2, 0, 1)
    return None


class GSplatDataset(torch.utils.data.Dataset):
    def __init__(self, path, resize_rate=1, device="cuda", masks=False, depths=False, normals=False,
                 normals_convention="opencv") -> None:
        super().__init__()
        from PIL import Image
        self.device = device
        self.resize_rate = resize_rate
        sparse = os.path.join(path, "sparse", "0")
        camera_params, image_params = colmap.read_model(sparse, ext=".bin")
        self.cameras, self.images = [], []
        self.weights = [] if masks else None
        self.depth_priors = [] if depths else None
        self.depth_kind = None
        self.normal_priors = [] if normals else None
        if normals_convention not in NORMALS_CONVENTIONS:
            raise ValueError("normals_convention must be one of %s, got %r" % (list(NORMALS_CONVENTIONS),
                                                                               normals_convention))
        depth_params = None
        if depths:
            fn = os.path.join(sparse, "depth_params.json")
            if os.path.exists(fn):
                with open(fn) as f:
                    depth_params = json.load(f)
            self.depth_kind = "metric" if depth_params is not None else "affine"
        for ip in image_params.values():
            cp = camera_params[ip.camera_id]
            im_path = os.path.join(path, "images", ip.name)
            image = Image.open(im_path)
            mask = _weight_source(path, ip.name, image) if masks else None
            if resize_rate != 1:
                image = image.resize((int(image.width * resize_rate), int(image.height * resize_rate)))
            if mask is not None and mask.size != image.size:      # (resized with the image; a mask of another size too)
                mask = mask.resize(image.size)
            w_scale, h_scale = image.width / cp.width, image.height / cp.height
            # the reference reads params[0..3] as fx, fy, cx, cy, i.e. it assumes a PINHOLE-like model
            # (gausplat_dataset.py:50-53); SIMPLE_* models store (f, cx, cy)
            if cp.model in ("SIMPLE_PINHOLE", "SIMPLE_RADIAL", "SIMPLE_RADIAL_FISHEYE", "RADIAL", "RADIAL_FISHEYE"):
                f, cx, cy = cp.params[0], cp.params[1], cp.params[2]
                fx, fy = f * w_scale, f * h_scale
                cx, cy = cx * w_scale, cy * h_scale
            else:
                fx, fy = cp.params[0] * w_scale, cp.params[1] * h_scale
                cx, cy = cp.params[2] * w_scale, cp.params[3] * h_scale
            Rcw = torch.from_numpy(ip.qvec2rotmat()).to(device).to(torch.float32)
            tcw = torch.from_numpy(np.asarray(ip.tvec)).to(device).to(torch.float32)
            self.cameras.append(Camera(ip.id, image.width, image.height, float(fx), float(fy), float(cx), float(cy),
                                       Rcw, tcw, im_path, device))
            self.images.append(_to_tensor(image, device))
            if masks:
                self.weights.append(None if mask is None else torch.from_numpy(np.array(mask, dtype=np.uint8)).to(device)
                                    .to(torch.float32).div_(255.0).contiguous())
            if depths:
                q = _depth_source(path, ip.name)
                if q is not None:
                    q = _nearest(q, image.width, image.height)
                    if depth_params is not None:
                        dp = depth_params.get(os.path.splitext(ip.name)[0])
                        if dp is None:      # (no alignment for this image: it cannot be used as a metric prior)
                            q = None
                        else:
                            q = np.where(q > 0, np.float32(dp["scale"]) * q + np.float32(dp["offset"]),
                                         np.float32(0)).astype(np.float32)
                self.depth_priors.append(None if q is None else
                                         torch.from_numpy(np.ascontiguousarray(q, np.float32)).to(device))
            if normals:
                nq = _normal_source(path, ip.name)
                if nq is not None:
                    nq = np.stack([_nearest(c, image.width, image.height) for c in nq])
                    if normals_convention == "opengl":      # (y up, z towards the viewer -> y down, z forward)
                        nq = nq * np.array([1, -1, -1], np.float32)[:, None, None]
                self.normal_priors.append(None if nq is None else
                                          torch.from_numpy(np.ascontiguousarray(nq, np.float32)).to(device))
        cache = os.path.join(sparse, "points3D.npy")
        if os.path.exists(cache):
            self.gs = np.load(cache)
        else:
            self.gs = colmap.read_points_bin_as_gau(os.path.join(sparse, "points3D.bin"))
            try:
                np.save(cache, self.gs)
            except OSError:
                pass                                   # read-only dataset directory
        twcs = torch.stack([c.twc for c in self.cameras])
        cam_dist = torch.linalg.norm(twcs - torch.mean(twcs, dim=0), dim=1)
        self.sence_size = float(torch.max(cam_dist)) * 1.1
        self.scene_size = self.sence_size

    def __getitem__(self, index: int):
        return self.cameras[index], self.images[index]

    def __len__(self) -> int:
        return len(self.images)
