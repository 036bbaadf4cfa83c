"""Render the animation of one blendshape-coefficient sequence on an MI355X.

Command-line compatible with the reference's script/render.py:23-96 (same twelve flags, types and defaults; `bool` flags keep argparse's
type=bool behaviour: any non-empty string turns them on), with these differences:
- --blendshape_list_path defaults to the 32 built-in names of said_amd/util/blendshape.py (the reference's default file lists the same names);
- the frames come from said_amd.render (HIP rasteriser) instead of pyrender / OpenGL: DESIGN.md section 15.  One sample per pixel by default;
  --samples 4 draws with four samples per pixel and a box resolve, as pyrender's multisampled offscreen target does (section 15.2);
- an --output_path ending in .avi is written by the built-in Motion-JPEG writer with the clip's sound as 16-bit PCM; any other extension goes
  through moviepy when it imports, and otherwise the .avi is written beside the requested path with a note on stderr;
- PNG frames (--save_images) are written with PIL, and --output_images_dir is created when missing;
- the reference passes R-G-B-reversed frames to moviepy (its renderer returns B-G-R for cv2.imwrite); with a grey material that is invisible,
  in difference mode it swaps red and blue in the video.  Here video and PNGs both show the colour map's own colours;
- new optional flags: --device, --chunk (frames per launch), --samples {1,4}, --jpeg {pil,gpu}: who encodes the .avi's frames, PIL on the host (default) or
  the HIP encoder on the device, after which only the compressed frames are copied to the host.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
if os.path.dirname(os.path.abspath(__file__)) not in sys.path:
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Render the animation")
    p.add_argument("--neutral_path", type=str, default="../BlendVOCA/templates_head/FaceTalk_170731_00024_TA.obj", help="Path of the neutral mesh")
    p.add_argument("--blendshapes_dir", type=str, default="../BlendVOCA/blendshapes_head/FaceTalk_170731_00024_TA", help="Directory of the blendshape meshes")
    p.add_argument("--audio_path", type=str, default="../BlendVOCA/audio/FaceTalk_170731_00024_TA/sentence01.wav", help="Path of the audio file")
    p.add_argument("--blendshape_coeffs_path", type=str, default="../BlendVOCA/blendshape_coeffs/FaceTalk_170731_00024_TA/sentence01.csv",
                   help="Path of the blendshape coefficient sequence")
    p.add_argument("--blendshape_list_path", type=str, default=None, help="List of the blendshapes (default: the 32 built-in ARKit names)")
    p.add_argument("--show_difference", type=bool, default=False, help="Show the vertex differences from the target blendshape coefficients as a heatmap")
    p.add_argument("--target_diff_blendshape_coeffs_path", type=str, default="../BlendVOCA/blendshape_coeffs/FaceTalk_170731_00024_TA/sentence01.csv",
                   help="Path of the target blendshape coefficient sequence to compute the vertex differences. Its length should be same as the source's.")
    p.add_argument("--max_diff", type=float, default=0.001, help="Maximum threshold to visualize the vertex differences")
    p.add_argument("--fps", type=int, default=60, help="FPS of the blendshape coefficients sequence")
    p.add_argument("--output_path", type=str, default="../out.mp4", help="Path of the output video file")
    p.add_argument("--save_images", type=bool, default=False, help="Save the image for each frame")
    p.add_argument("--output_images_dir", type=str, default="../out_imgs", help="Saving directory of the output image for each frame")
    p.add_argument("--device", type=str, default="cuda:0", help="MI355X to run on")
    p.add_argument("--chunk", type=int, default=64, help="Frames rendered per launch")
    p.add_argument("--samples", type=int, choices=[1, 4], default=1, help="Samples per pixel: 1, or 4 with a box resolve (smooth silhouettes)")
    p.add_argument("--jpeg", choices=["pil", "gpu"], default="pil", help="JPEG encoder of the video's frames: PIL on the host, or the HIP encoder on the device")
    return p


def main(argv=None) -> None:
    args = build_parser().parse_args(argv)
    from PIL import Image

    from _common import load_blendshape_basis, write_video
    from said_amd.render import RendererObject, iter_encoded_frames, iter_rendered_frames
    from said_amd.util.blendshape import DEFAULT_BLENDSHAPE_CLASSES, load_blendshape_coeffs
    from said_amd.util.parser import parse_list

    names = parse_list(args.blendshape_list_path, str) if args.blendshape_list_path else list(DEFAULT_BLENDSHAPE_CLASSES)
    neutral, basis = load_blendshape_basis(args.neutral_path, args.blendshapes_dir, names)
    coeffs = load_blendshape_coeffs(args.blendshape_coeffs_path).numpy()
    target = load_blendshape_coeffs(args.target_diff_blendshape_coeffs_path).numpy() if args.show_difference else None
    renderer = RendererObject(device=args.device, samples=args.samples)
    if args.jpeg == "gpu":   # the PNGs of --save_images need the pixels as well
        frames = iter_encoded_frames(renderer, neutral, basis, coeffs, target, max_diff=args.max_diff, chunk=args.chunk, raw=bool(args.save_images))
    else:
        frames = iter_rendered_frames(renderer, neutral, basis, coeffs, target, max_diff=args.max_diff, chunk=args.chunk)

    on_frame = None
    if args.save_images:
        os.makedirs(args.output_images_dir, exist_ok=True)

        def on_frame(index, frame):
            Image.fromarray(frame[..., ::-1].copy(), "RGB").save(os.path.join(args.output_images_dir, f"{index}.png"))

    written = write_video(frames, args.output_path, args.fps, args.audio_path, on_frame=on_frame, encoded=args.jpeg == "gpu")
    print(f"{len(coeffs)} frames -> {written}")
    renderer.close()


if __name__ == "__main__":
    main()
