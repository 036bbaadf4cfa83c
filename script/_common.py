"""Pieces shared by the two command-line drivers (script/inference.py, script/test_inference.py).

The flag NAMES, TYPES and DEFAULTS are the drop-in contract with the reference CLIs
(/root/reference/script/inference.py:23-117, script/test_inference.py:23-126); they are kept in one table here.
Everything behind them is this repository's own: the model is said_amd's (HIP engine, no CPU path), WAV files are read
with scipy, and `--weights_path synthetic` selects the deterministic test weights (no checkpoint is reachable offline).
"""
import argparse
import os
import sys
from typing import Iterable, Tuple

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from said_amd.model.diffusion import SAID_UNet1D  # noqa: E402
from said_amd.scheduler import SCHEDULERS, DDIMScheduler  # noqa: E402
from said_amd.util.audio import fit_audio_unet, load_audio  # noqa: E402

# flag -> (type, default, description).  `bool` flags keep argparse's type=bool behaviour of the reference
# (any non-empty string, including "False", turns them on).
FLAG_TABLE = {
    "weights_path": (str, "../BlendVOCA/SAiD.pth", "checkpoint with the SAID_UNet1D state dict, or 'synthetic' for the seeded test weights"),
    "audio_path": (str, "../BlendVOCA/audio/FaceTalk_170731_00024_TA/sentence01.wav", "input speech, WAV"),
    "audio_dir": (str, "../BlendVOCA/audio", "root of <person_id>/sentenceNN.wav inputs"),
    "output_path": (str, "../out.csv", "where the (frames x 32) coefficient table is written"),
    "output_dir": (str, "../output-inference", "root of <person_id>/sentenceNN-<repeat>.csv outputs"),
    "output_image_path": (str, "../out.png", "heat-map rendering of the coefficients (with --save_image)"),
    "intermediate_dir": (str, "../interm", "one CSV + PNG per denoising step goes here (with --save_intermediate)"),
    "prediction_type": (str, "epsilon", "what the denoiser predicts: epsilon | sample | v_prediction"),
    "save_image": (bool, False, "also render the result as an image"),
    "save_intermediate": (bool, False, "also dump the latents before every step"),
    "num_steps": (int, 1000, "denoising steps"),
    "strength": (float, 1.0, "fraction of the schedule to run when editing an initial sample"),
    "guidance_scale": (float, 2.0, "classifier-free guidance weight (<= 1 disables guidance)"),
    "guidance_rescale": (float, 0.0, "rescale_noise_cfg blend factor"),
    "eta": (float, 0.0, "DDIM stochasticity in [0, 1]"),
    "fps": (int, 60, "coefficient frames per second"),
    "divisor_unet": (int, 1, "pad the audio so that the frame count is a multiple of this"),
    "unet_feature_dim": (int, -1, "width of the projected audio features (-1: use the 768 encoder features)"),
    "device": (str, "cuda:0", "the MI355X to run on"),
    "init_sample_path": (str, None, "CSV of coefficients to start from (editing)"),
    "mask_path": (str, None, "CSV mask, 1 = keep the initial sample there"),
    "num_repeats": (int, 72, "samples to draw per audio clip"),
    "batch_size": (int, 64, "samples per batch"),
    "seed": (int, 0, "torch seed; negative = leave the generator alone"),
}


def parser_with(description: str, names: Iterable[str]) -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description=description)
    for name in names:
        typ, default, text = FLAG_TABLE[name]
        ap.add_argument("--" + name, type=typ, default=default, help=text)
    # Not a reference flag: the reference selects its sampler in code (the noise_scheduler slot of SAID).  Both drivers get it here.
    ap.add_argument("--scheduler", choices=sorted(SCHEDULERS), default="ddim",
                    help="sampler: ddim (default), ddpm or dpmsolver++ (DPM-Solver++(2M)); --eta only affects ddim")
    return ap


def make_model(args) -> SAID_UNet1D:
    """SAID_UNet1D on args.device with the weights named by --weights_path, in eval mode."""
    net = SAID_UNet1D(noise_scheduler=DDIMScheduler, feature_dim=args.unet_feature_dim, prediction_type=args.prediction_type)
    if args.weights_path == "synthetic":
        from said_amd.util import synth
        state = synth.said_state_dict()
    else:
        state = torch.load(args.weights_path, map_location="cpu")
    net.load_state_dict(state, strict=True)
    name = getattr(args, "scheduler", "ddim")
    if name != "ddim":   # SAID_UNet1D does not forward noise_scheduler (as in the reference): set the slot itself
        net.noise_scheduler = SCHEDULERS[name](num_train_timesteps=1000, beta_schedule="squaredcos_cap_v2", prediction_type=args.prediction_type)
    return net.to(args.device).eval()


def prepared_audio(net: SAID_UNet1D, path: str, fps: int, divisor: int) -> Tuple[torch.Tensor, int]:
    """(1, Ta) normalised waveform on the model's device, padded for the UNet, and the number of frames to keep."""
    fitted = fit_audio_unet(load_audio(path, net.sampling_rate), net.sampling_rate, fps, divisor)
    return net.process_audio(fitted.waveform).to(next(net.parameters()).device), fitted.window_size


# ---- rendering (script/render.py, script/test_render.py)
def load_blendshape_basis(neutral_path: str, blendshapes_dir: str, names):
    """(neutral mesh, (3V, K) matrix [b_1 | ... | b_K]) from <neutral_path> and <blendshapes_dir>/<name>.obj, as the reference's drivers build them."""
    import numpy as np
    from said_amd.util.mesh import load_mesh, load_vertices
    neutral = load_mesh(neutral_path)
    cols = []
    for name in names:
        v = load_vertices(os.path.join(blendshapes_dir, f"{name}.obj"))
        if v.shape != neutral.vertices.shape:
            raise ValueError(f"blendshape {name} has {len(v)} vertices, the neutral mesh {len(neutral.vertices)}")
        cols.append(v.reshape(-1, 1))
    return neutral, np.concatenate(cols, axis=1)


def _decoded_chunks(encoded_iter):
    """Chunks of JPEG files (or (files, frames) pairs) -> chunks of B-G-R frames, for a writer that wants pixels."""
    import io

    import numpy as np
    from PIL import Image
    for chunk in encoded_iter:
        files, pixels = chunk if isinstance(chunk, tuple) else (chunk, None)
        yield pixels if pixels is not None else [np.asarray(Image.open(io.BytesIO(f)).convert("RGB"))[..., ::-1] for f in files]


def write_video(frames_iter, output_path: str, fps: int, audio_path: str, width: int = 800, height: int = 800, on_frame=None, encoded: bool = False) -> str:
    """Stream B-G-R frame chunks and the sound of audio_path into a video; returns the path written.  A path ending in .avi gets the built-in
    Motion-JPEG writer (said_amd/util/video.py).  Any other extension needs moviepy (and its ffmpeg): when it does not import, the .avi is
    written beside the requested path and stderr says so, rather than failing after the frames were rendered.
    With `encoded`, frames_iter yields chunks that are already JPEG files (said_amd.render.iter_encoded_frames): lists of bytes, or pairs
    (files, frames) when on_frame needs the pixels.  They go into the .avi as they are; moviepy, which wants pixels, gets them decoded."""
    import numpy as np
    from said_amd.util.video import AviWriter
    want_avi = output_path.lower().endswith(".avi")
    mpy = None
    if not want_avi:
        try:
            from moviepy import editor as mpy   # noqa: F401
        except Exception:
            mpy = None
            fallback = os.path.splitext(output_path)[0] + ".avi"
            print(f"moviepy is not importable: writing Motion-JPEG AVI to {fallback} instead of {output_path}", file=sys.stderr)
            output_path, want_avi = fallback, True
    os.makedirs(os.path.dirname(os.path.abspath(output_path)), exist_ok=True)
    index = 0
    if want_avi:
        audio = rate = None
        if audio_path:
            from scipy.io import wavfile
            rate, audio = wavfile.read(audio_path)
            if audio.dtype != np.int16:
                from said_amd.util.video import pcm16
                audio = pcm16(audio.astype(np.float64) / (np.iinfo(audio.dtype).max if audio.dtype.kind in "iu" else 1.0))
        with AviWriter(output_path, fps, width, height, audio=audio, audio_rate=rate) as out:
            for chunk in frames_iter:
                files, pixels = (chunk if isinstance(chunk, tuple) else (chunk, None)) if encoded else (None, chunk)
                if on_frame is not None and pixels is None:
                    raise ValueError("on_frame needs the pixels: ask iter_encoded_frames for raw=True")
                for i in range(len(files if encoded else pixels)):
                    if encoded:
                        out.write_encoded(files[i])
                    else:
                        out.write(pixels[i])
                    if on_frame is not None:
                        on_frame(index, pixels[i])
                    index += 1
        return output_path
    if encoded:
        frames_iter = _decoded_chunks(frames_iter)
    frames = []
    for chunk in frames_iter:   # moviepy's ImageSequenceClip wants the whole list, R-G-B
        for frame in chunk:
            frames.append(frame[..., ::-1].copy())
            if on_frame is not None:
                on_frame(index, frame)
            index += 1
    audio_clip = mpy.AudioFileClip(audio_path)
    clip = mpy.ImageSequenceClip(frames, fps=fps).set_audio(audio_clip)
    clip.write_videofile(output_path, fps=fps, logger=None)
    audio_clip.close()
    clip.close()
    return output_path
