"""Render every coefficient sequence of the evaluation set on an MI355X.

Command-line compatible with the reference's script/test_render.py:25-74 (same eight flags, types and defaults), with the differences of
script/render.py: the built-in blendshape names when --blendshape_list_path is not given, said_amd.render instead of pyrender, and videos
through the built-in Motion-JPEG writer unless moviepy imports (--video_ext picks the extension; the reference writes .mp4).

Files are enumerated as BlendVOCAEvalDataset.get_data_paths does (script/dataset/dataset_voca.py:175-241): the two test speakers, sentences
1..40 that have <audio_dir>/<person>/sentenceNN.wav, and every <coeffs_dir>/<person>/sentenceNN<repeat_regex>.csv; the output is
<output_dir>/<person>/<csv stem>.<ext>.  A person's mesh is uploaded once.
"""
import argparse
import os
import pathlib
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
if os.path.dirname(os.path.abspath(__file__)) not in sys.path:
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

PERSON_IDS_TEST = ["FaceTalk_170731_00024_TA", "FaceTalk_170809_00138_TA"]   # script/dataset/dataset_voca.py:90-93
SENTENCE_IDS = list(range(1, 41))


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Render the animation of the dataset")
    p.add_argument("--neutral_dir", type=str, default="../BlendVOCA/templates_head", help="Directory of the neutral mesh data")
    p.add_argument("--audio_dir", type=str, default="../BlendVOCA/audio", help="Directory of the audio data")
    p.add_argument("--coeffs_dir", type=str, default="../BlendVOCA/blendshape_coeffs", help="Directory of the blendshape coefficients data")
    p.add_argument("--blendshapes_dir", type=str, default="../BlendVOCA/blendshapes_head", help="Directory of the blendshape meshes")
    p.add_argument("--blendshape_list_path", type=str, default=None, help="List of the blendshapes (default: the 32 built-in ARKit names)")
    p.add_argument("--fps", type=int, default=60, help="FPS of the blendshape coefficients sequence")
    p.add_argument("--repeat_regex", type=str, default="(-.+)?", help="Regex for checking the repeated files")
    p.add_argument("--output_dir", type=str, default="../out_render", help="Saving directory of the output video files")
    p.add_argument("--video_ext", type=str, default="mp4", help="Extension of the videos; avi selects the built-in Motion-JPEG writer")
    p.add_argument("--device", type=str, default="cuda:0", help="MI355X to run on")
    p.add_argument("--chunk", type=int, default=64, help="Frames rendered per launch")
    return p


def get_data_paths(audio_dir: str, coeffs_dir: str, repeat_regex: str):
    """(person_id, audio path, csv path) in the reference's order."""
    out = []
    for pid in PERSON_IDS_TEST:
        cdir = os.path.join(coeffs_dir, pid)
        for sid in SENTENCE_IDS:
            base = f"sentence{sid:02}"
            audio = os.path.join(audio_dir, pid, f"{base}.wav")
            if not os.path.exists(audio) or not os.path.isdir(cdir):
                continue
            pattern = re.compile(f"^{base}{repeat_regex}\\.csv$")
            out += [(pid, audio, os.path.join(cdir, s)) for s in os.listdir(cdir) if pattern.match(s)]
    return out


def main(argv=None) -> None:
    args = build_parser().parse_args(argv)
    from _common import load_blendshape_basis, write_video
    from said_amd.render import RendererObject, iter_rendered_frames
    from said_amd.util.blendshape import DEFAULT_BLENDSHAPE_CLASSES, load_blendshape_coeffs
    from said_amd.util.parser import parse_list

    names = parse_list(args.blendshape_list_path, str) if args.blendshape_list_path else list(DEFAULT_BLENDSHAPE_CLASSES)
    renderer = RendererObject(device=args.device)
    meshes = {}
    for pid, audio, csv in get_data_paths(args.audio_dir, args.coeffs_dir, args.repeat_regex):
        if pid not in meshes:
            meshes[pid] = load_blendshape_basis(os.path.join(args.neutral_dir, f"{pid}.obj"), os.path.join(args.blendshapes_dir, pid), names)
        neutral, basis = meshes[pid]
        out = os.path.join(args.output_dir, pid, f"{pathlib.Path(csv).stem}.{args.video_ext}")
        coeffs = load_blendshape_coeffs(csv).numpy()
        written = write_video(iter_rendered_frames(renderer, neutral, basis, coeffs, chunk=args.chunk), out, args.fps, audio)
        print(f"{csv}: {len(coeffs)} frames -> {written}")
    renderer.close()


if __name__ == "__main__":
    main()
