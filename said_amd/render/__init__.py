"""Render blendshape animation on the GPU (reference: script/rendering/render_visual.py; kernels: csrc/render.hip).

``RendererObject`` holds the reference's scene (its camera, four point lights, ambient term and material) and a ``RenderEngine``;
``render_blendshape_coefficients`` returns the list of (800, 800, 3) uint8 B-G-R images the reference returns, and
``iter_rendered_frames`` yields the same images chunk by chunk, so a long clip never holds all its frames on the device.
``RendererObject(samples=4)`` draws with four samples per pixel and a box resolve, as pyrender's offscreen target
does; the default is one sample.  There is no CPU path."""
from __future__ import annotations

from typing import Iterator, List, Optional

import numpy as np
import torch

from .._engine import RENDER_LUT, EngineError, JpegEngine, RenderEngine, RenderScene

WIDTH = HEIGHT = 800
FOCAL = 4754.97941935 / 2
ZNEAR, ZFAR = 0.01, 3.0
LIGHT_INTENSITY, AMBIENT = 2.0, 0.2
BASE_COLOR, METALLIC, ROUGHNESS = 0.3, 0.8, 0.8
VC_METALLIC, VC_ROUGHNESS = 1.0, 1.0   # pyrender's default material, used when vertex colours are drawn
DEFAULT_CHUNK = 64                     # frames per launch: 64 x 1.92 MB = 123 MB of pixels


def rodrigues(rvec) -> np.ndarray:
    """(3, 3) rotation matrix of an axis-angle vector (what cv2.Rodrigues(rvec)[0] returns), float64."""
    r = np.asarray(rvec, dtype=np.float64).reshape(3)
    t = float(np.sqrt(r @ r))
    if t == 0.0:
        return np.eye(3)
    x, y, z = r / t
    k = np.array([[0.0, -z, y], [z, 0.0, -x], [-y, x, 0.0]])
    return np.eye(3) + np.sin(t) * k + (1.0 - np.cos(t)) * (k @ k)


def light_positions(z_offset: float = 0.0) -> np.ndarray:
    """(4, 3): pos = (0, 0, 1 - z_offset) and its rotations by +pi/6 and -pi/6 about x and -pi/6 about y (render_visual.py:61-77)."""
    pos = np.array([0.0, 0.0, 1.0 - z_offset])
    a = np.pi / 6.0
    return np.stack([pos, rodrigues([a, 0, 0]) @ pos, rodrigues([-a, 0, 0]) @ pos, rodrigues([0, -a, 0]) @ pos])


def colormap_index(x: np.ndarray, n: int = RENDER_LUT) -> np.ndarray:
    """matplotlib's bin of x in [0, 1]: int(x n), with x == 1 in the last bin (matplotlib.colors.Colormap.__call__)."""
    x = np.asarray(x, dtype=np.float64)
    return np.clip(np.where(x >= 1.0, n - 1, (x * n).astype(np.int64)), 0, n - 1)


def colormap_table(color_map: str = "viridis") -> np.ndarray:
    """(256, 3) float32 RGB of matplotlib.colormaps[color_map] at its 256 bins, as 8-bit levels / 255: trimesh keeps vertex colours as uint8,
    so that is what the reference's shader receives."""
    import matplotlib
    cmap = matplotlib.colormaps[color_map]
    lut = np.asarray(cmap(np.arange(RENDER_LUT) if cmap.N == RENDER_LUT else np.linspace(0.0, 1.0, RENDER_LUT)), dtype=np.float64)[:, :3]
    return (np.round(lut * 255.0) / 255.0).astype(np.float32)


class RendererObject:
    """The reference's scene.  The camera stands at (0, 0, 1) whatever z_offset is: the reference computes a camera pose from z_offset and then
    adds the camera with a literal pose, so z_offset moves the four lights only.  That quirk is kept."""

    def __init__(self, z_offset: float = 0.0, device="cuda:0", samples: int = 1) -> None:
        if samples not in (1, 4):
            raise ValueError(f"samples must be 1 or 4, got {samples}")
        self.z_offset = float(z_offset)
        self.samples = int(samples)   # per pixel, used by the frame iterators below
        self.frustum = {"near": ZNEAR, "far": ZFAR, "height": HEIGHT, "width": WIDTH}
        self.engine = RenderEngine(torch.device(device))
        self.device = self.engine.device
        sc = RenderScene()
        sc.width, sc.height = WIDTH, HEIGHT
        sc.fx = sc.fy = FOCAL
        sc.cx = sc.cy = 400.0
        sc.znear, sc.zfar = ZNEAR, ZFAR
        sc.cam_pos[:] = [0.0, 0.0, 1.0]
        lights = light_positions(self.z_offset)
        sc.n_lights = len(lights)
        for i, p in enumerate(lights):
            sc.light_pos[i][:] = [float(v) for v in p]
            sc.light_intensity[i] = LIGHT_INTENSITY
        sc.ambient = AMBIENT
        sc.base_color[:] = [BASE_COLOR] * 3
        sc.metallic, sc.roughness, sc.vc_metallic, sc.vc_roughness = METALLIC, ROUGHNESS, VC_METALLIC, VC_ROUGHNESS
        self.scene = sc
        self.engine.set_scene(sc)
        self._mesh_key = None
        self._cmap = None
        self._jpeg = None   # the JpegEncoder iter_encoded_frames keeps here, one per size and quality

    def set_mesh(self, vertices, faces, blendshapes_matrix) -> None:
        self._mesh_key = None
        self.engine.set_mesh(vertices, faces, blendshapes_matrix)

    def set_colormap(self, color_map: str) -> None:
        if self._cmap != color_map:
            self.engine.set_colormap(colormap_table(color_map))
            self._cmap = color_map

    def close(self) -> None:
        if self._jpeg is not None:
            self._jpeg.close()
            self._jpeg = None
        self.engine.close()


def _device_coeffs(a, device, name: str) -> torch.Tensor:
    t = torch.as_tensor(np.asarray(a, dtype=np.float32) if not isinstance(a, torch.Tensor) else a, dtype=torch.float32)
    if t.dim() != 2:
        raise ValueError(f"{name} must be (T, num_blendshapes), got {tuple(t.shape)}")
    return t.to(device).contiguous()


def _prepare_sequence(renderer: RendererObject, neutral_mesh, blendshapes_matrix, blendshape_coeffs, target_blendshape_coeffs, color_map: str, t_center):
    """What both frame iterators do before their first chunk: the mesh upload (skipped when the same mesh is drawn again), the coefficient
    sequences on the device, the colour map of a difference render, and the rotation centre.  Returns (coeffs, target or None, center)."""
    eng = renderer.engine
    verts = np.asarray(neutral_mesh.vertices, dtype=np.float64)
    faces = np.asarray(neutral_mesh.faces)
    basis = np.ascontiguousarray(blendshapes_matrix, dtype=np.float64)
    key = hash((verts.tobytes(), faces.tobytes(), basis.tobytes()))
    if renderer._mesh_key != key:   # the upload is skipped when the same mesh is drawn again (script/test_render.py: one per person)
        renderer.set_mesh(verts, faces, basis)
        renderer._mesh_key = key
    coeffs = _device_coeffs(blendshape_coeffs, eng.device, "blendshape_coeffs")
    target = None
    if target_blendshape_coeffs is not None:
        target = _device_coeffs(target_blendshape_coeffs, eng.device, "target_blendshape_coeffs")
        if target.shape != coeffs.shape:
            raise ValueError(f"target_blendshape_coeffs {tuple(target.shape)} and blendshape_coeffs {tuple(coeffs.shape)} differ in shape")
        renderer.set_colormap(color_map)
    center = verts.mean(axis=0) if t_center is None else np.asarray(t_center, dtype=np.float64)
    return coeffs, target, center


def iter_rendered_frames(renderer: RendererObject, neutral_mesh, blendshapes_matrix: np.ndarray, blendshape_coeffs, target_blendshape_coeffs=None,
                         color_map: str = "viridis", max_diff: float = 0.001, chunk: int = DEFAULT_CHUNK, rot=None, t_center=None,
                         face_ids: bool = False) -> Iterator[np.ndarray]:
    """Yields (n, 800, 800, 3) uint8 B-G-R arrays, n <= chunk frames at a time, in order (with face_ids: pairs (frames, (n, 800, 800) int32);
    a renderer of 4 samples gives the face of every sample instead, (n, 800, 800, 4) int32).
    The arrays are views of one pinned host buffer that the next chunk overwrites: copy what must outlive the iteration step.
    `t_center` defaults to the mean of the neutral vertices, as in the reference; `rot` (axis-angle) to no rotation."""
    if chunk < 1:
        raise ValueError("chunk must be at least 1")
    eng = renderer.engine
    coeffs, target, center = _prepare_sequence(renderer, neutral_mesh, blendshapes_matrix, blendshape_coeffs, target_blendshape_coeffs, color_map, t_center)
    T = coeffs.shape[0]
    n_max = min(chunk, T)
    if n_max == 0:
        return
    h, w = eng.height, eng.width
    with torch.cuda.device(eng.index):
        dev = torch.empty((n_max, h, w, 3), dtype=torch.uint8, device=eng.device)
        host = torch.empty((n_max, h, w, 3), dtype=torch.uint8, pin_memory=True)
        ms = renderer.samples != 1
        ids_dev = torch.empty((n_max, h, w, 4) if ms else (n_max, h, w), dtype=torch.int32, device=eng.device) if face_ids else None
        for t0 in range(0, T, chunk):
            n = min(chunk, T - t0)
            eng.render(coeffs, t0, n, dev, target=target, max_diff=max_diff, rot=rot, t_center=center, face_ids=None if ms else ids_dev,
                       samples=renderer.samples, sample_ids=ids_dev if ms else None)
            host[:n].copy_(dev[:n], non_blocking=True)
            ids = ids_dev[:n].cpu() if face_ids else None
            torch.cuda.current_stream().synchronize()
            frames = host[:n].numpy()
            yield (frames, ids.numpy()) if face_ids else frames


def render_blendshape_coefficients(renderer: RendererObject, neutral_mesh, blendshapes_matrix: np.ndarray, blendshape_coeffs,
                                   target_blendshape_coeffs=None, color_map: str = "viridis", max_diff: float = 0.001,
                                   chunk: int = DEFAULT_CHUNK) -> List[np.ndarray]:
    """The reference's render_blendshape_coefficients: one (800, 800, 3) uint8 B-G-R image per row of blendshape_coeffs."""
    out: List[np.ndarray] = []
    for frames in iter_rendered_frames(renderer, neutral_mesh, blendshapes_matrix, blendshape_coeffs, target_blendshape_coeffs, color_map, max_diff, chunk):
        out.extend(frames.copy())
    return out


class JpegEncoder:
    """Baseline JPEG files of device frames (include/said_jpeg.h): ``encode`` takes an (n, height, width, 3) uint8 tensor
    on the device (a numpy array is uploaded) and returns one complete JFIF file per frame.  Only the compressed bytes travel to the host."""

    def __init__(self, device, width: int, height: int, quality: int = 90) -> None:
        self.engine = JpegEngine(torch.device(device), width, height, quality)
        self.device, self.width, self.height, self.quality = self.engine.device, int(width), int(height), int(quality)
        self.header = self.engine.header
        self._out = self._host = self._offsets = None

    def _room(self, n: int, capacity: int) -> None:
        dev = torch.device("cuda", self.engine.index)
        if self._out is None or self._out.numel() < capacity:
            self._out = torch.empty(capacity, dtype=torch.uint8, device=dev)
            self._host = torch.empty(capacity, dtype=torch.uint8, pin_memory=True)
        if self._offsets is None or self._offsets.numel() < n + 1:
            self._offsets = torch.empty(n + 1, dtype=torch.int64, device=dev)

    def encode(self, frames, bgr: bool = True) -> List[bytes]:
        if not isinstance(frames, torch.Tensor):
            frames = torch.from_numpy(np.ascontiguousarray(frames))
        if frames.dim() == 3:
            frames = frames[None]
        if frames.dim() != 4 or tuple(frames.shape[1:]) != (self.height, self.width, 3) or frames.dtype != torch.uint8:
            raise ValueError(f"frames must be (n, {self.height}, {self.width}, 3) uint8, got {tuple(frames.shape)} {frames.dtype}")
        n = frames.shape[0]
        if n == 0:
            return []
        eng = self.engine
        with torch.cuda.device(eng.index):
            frames = frames.to(torch.device("cuda", eng.index)).contiguous()
            # a quarter of the raw size to start with (rendered frames compress about sixty times); one retry at the size the encoder reports
            self._room(n, max(frames.numel() // 4, 1))
            fits, total = eng.encode(frames, n, self._out, self._offsets, bgr=bgr)
            if not fits:
                self._room(n, total)
                fits, total = eng.encode(frames, n, self._out, self._offsets, bgr=bgr)
                if not fits:
                    raise EngineError(f"said_jpeg_encode: {total} bytes required twice over a buffer of that size")
            self._host[:total].copy_(self._out[:total], non_blocking=True)   # only the used bytes
            offsets = self._offsets[:n + 1].cpu().tolist()                    # synchronises the stream: the copy above has landed
            torch.cuda.current_stream().synchronize()
        data = self._host[:total].numpy().tobytes()
        return [self.header + data[offsets[i]:offsets[i + 1]] for i in range(n)]

    def close(self) -> None:
        self.engine.close()


def iter_encoded_frames(renderer: RendererObject, neutral_mesh, blendshapes_matrix: np.ndarray, blendshape_coeffs, target_blendshape_coeffs=None,
                        color_map: str = "viridis", max_diff: float = 0.001, chunk: int = DEFAULT_CHUNK, rot=None, t_center=None,
                        face_ids: bool = False, quality: int = 90, raw: bool = False):
    """``iter_rendered_frames`` with the JPEG encoding done on the device: yields, per chunk, the list of its frames' JPEG files (bytes).  With
    ``raw`` it yields (files, frames), the frames as ``iter_rendered_frames`` gives them (views of a buffer the next chunk overwrites);
    without it no pixel leaves the device.  ``face_ids`` is accepted for the signature's sake and must be False."""
    if face_ids:
        raise ValueError("iter_encoded_frames yields JPEG files; face ids come from iter_rendered_frames")
    if chunk < 1:
        raise ValueError("chunk must be at least 1")
    eng = renderer.engine
    coeffs, target, center = _prepare_sequence(renderer, neutral_mesh, blendshapes_matrix, blendshape_coeffs, target_blendshape_coeffs, color_map, t_center)
    T = coeffs.shape[0]
    n_max = min(chunk, T)
    if n_max == 0:
        return
    h, w = eng.height, eng.width
    enc = renderer._jpeg
    if enc is None or (enc.width, enc.height, enc.quality) != (w, h, int(quality)):
        if enc is not None:
            enc.close()
        enc = renderer._jpeg = JpegEncoder(eng.device, w, h, quality)
    with torch.cuda.device(eng.index):
        dev = torch.empty((n_max, h, w, 3), dtype=torch.uint8, device=eng.device)
        host = torch.empty((n_max, h, w, 3), dtype=torch.uint8, pin_memory=True) if raw else None
        for t0 in range(0, T, chunk):
            n = min(chunk, T - t0)
            eng.render(coeffs, t0, n, dev, target=target, max_diff=max_diff, rot=rot, t_center=center, samples=renderer.samples)
            if raw:
                host[:n].copy_(dev[:n], non_blocking=True)
            files = enc.encode(dev[:n], bgr=True)   # synchronises the stream
            yield (files, host[:n].numpy()) if raw else files


__all__ = ["RendererObject", "render_blendshape_coefficients", "iter_rendered_frames", "iter_encoded_frames", "JpegEncoder", "rodrigues",
           "light_positions", "colormap_index", "colormap_table", "EngineError"]
