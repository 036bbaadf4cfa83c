"""The host side of rendering with 4 samples per pixel: the restatement's own ambiguity cap on the scenes the GPU
test renders, the CLIs' --samples flag and the resolve rule."""
import importlib.util
import os

import numpy as np

import render_ms_ref as ms
import render_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ambiguous_pixels_stay_under_the_cap():
    """On the two full 800 x 800 scenes of tests/test_gpu_render_ms.py the restatement's ambiguous pixels (any sample within 1e-4 px of a
    deciding edge or 1e-6 of a depth tie, or a shade extrapolated beyond |b| = 16) are under 0.1 % of the pixels with any covered sample."""
    neutral, basis, faces = rr.arkit_mesh(os.path.join(ROOT, "tests", "golden"))
    w, _ = rr.scene_coeffs()
    verts = rr.blend(neutral, basis, w)
    sc = rr.scene()
    for t, rot in ms.SCENES:
        out = ms.render_frame_ms(verts[t], faces, sc, rot=rot, t_center=neutral.mean(axis=0))
        covered = int((out["face"] >= 0).any(axis=-1).sum())
        ambiguous = int(out["ambiguous"].sum())
        mixed = int((out["face"].min(axis=-1) != out["face"].max(axis=-1)).sum())
        print(f"frame {t} rot {rot}: {ambiguous} ambiguous of {covered} covered pixels, {mixed} with two or more sample values, max |b| {out['max_b']:.2f}")
        assert covered > 100000 and mixed > 10000
        assert out["max_b"] <= ms.MAX_BARY   # the |b| rule flags nothing on these scenes
        assert ambiguous < 1e-3 * covered


def load_script(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "script", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_cli_samples_flag():
    """script/render.py has --samples with default 1 and choices {1, 4}.  (script/test_render.py is not changed and has no such flag.)"""
    parser = load_script("render").build_parser()
    action = {a.dest: a for a in parser._actions}["samples"]
    assert action.type is int and action.default == 1 and set(action.choices) == {1, 4}
    assert parser.parse_args([]).samples == 1 and parser.parse_args(["--samples", "4"]).samples == 4


def test_resolve_rule():
    """(c0 + c1 + c2 + c3 + 2) >> 2 per channel, on hand-written sample bytes."""
    samples = np.array([
        [[0, 0, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0]],                  # nothing covered
        [[255, 255, 255]] * 4,                                         # the same value four times is that value
        [[51, 128, 230], [51, 128, 230], [51, 128, 230], [0, 0, 0]],   # three covered: (153 + 2) >> 2, (384 + 2) >> 2, (690 + 2) >> 2
        [[51, 128, 230], [0, 0, 0], [0, 0, 0], [0, 0, 0]],             # one covered
        [[1, 2, 3], [0, 0, 0], [0, 0, 0], [0, 0, 0]],                  # 3 >> 2, 4 >> 2, 5 >> 2: halves round up
        [[10, 20, 255], [11, 21, 255], [10, 21, 254], [11, 20, 255]],  # 44 >> 2, 84 >> 2, 1021 >> 2
    ], dtype=np.uint8)
    want = [[0, 0, 0], [255, 255, 255], [38, 96, 173], [13, 32, 58], [0, 1, 1], [11, 21, 255]]
    got = ms.resolve(samples)
    assert got.dtype == np.uint8 and got.tolist() == want
    rng = np.random.default_rng(4)
    s = rng.integers(0, 256, size=(1000, 4, 3), dtype=np.uint8)
    assert np.array_equal(ms.resolve(s), np.floor(s.astype(np.float64).mean(axis=1) + 0.5).astype(np.uint8))
    assert np.array_equal(ms.resolve(np.repeat(s[:, :1], 4, axis=1)), s[:, 0])   # four samples of one face: that face's bytes
