#!/usr/bin/env python
"""tools/w2xc_cli.py -- N4: a parity shell for the reference CLI (/root/reference/src/main.cpp) on top of
libw2xc_hip, for machines without OpenCV.  Same flags (main.cpp:26-60), same mode / ratio logic
(:83-121, iter = ceil(log2 ratio), shrink iff int(ratio) != 2^iter, :107-114,158-167), same automatic output
name (:173-189).  Image I/O is PIL instead of cv::imread/imwrite; everything between -- convertTo,
RGB2YUV on BGR data (Q3), noise pass, nearest/bicubic 2x + CNN, linear shrink, YUV2RGB, saturate to uint8 --
runs on the GPU in one call (w2xc_process_image_u8_ex).
Extension: several input files (-i a.png b.png ...).  They are grouped by image size and every group is ONE w2xc_process_image_u8_batch call; each
output gets its automatic name (-o is for a single input only).  A single input behaves exactly as before.
Extension: RGB models.  When the loaded model's first layer takes 3 planes the image goes through w2xc_process_image_rgb_u8_ex / _batch instead: the three
channels in PIL's RGB order as they are (no BGR swap: that mimics what the reference feeds its Y path), all three planes through the CNN.
Extension: transparency.  An input whose decoded image has an alpha channel with any byte below 255 (PIL modes RGBA, LA, P with transparency, ...) goes through
w2xc_process_image_rgba_u8_ex on the route of the models -- the colour bled under the transparent pixels, alpha through the scale model -- and is written as
RGBA; several such inputs are grouped by image size like the opaque ones, and a group of two or more is ONE w2xc_process_image_rgba_u8_batch call.  Every
other input goes exactly as before, the batch grouping included.
Extension: -t/--tta 1 = test-time augmentation, the --tta of later upstream versions: every model pass on the 8 flips / transposes of the image, averaged
(w2xc_process_image_[rgb_]u8[_batch]_tta; 8x the CNN work), on both routes and for grouped inputs.  With an input that would take the RGBA call, --tta 1
alone exits with a message before anything is converted; --tta 1 --tta_alpha 1 opts in: such inputs go to the TTA forms of the RGBA calls
(w2xc_process_image_rgba_u8[_up2x]_batch_tta: colour AND alpha through 8 variants per pass), one call per size group (alpha_tta_routes).
Extension: upconv scale models (upconv_7: the model enlarges by itself).  The RGB route; a size group of two or more opaque inputs, and every input under
--tta 1, is ONE w2xc_process_image_rgb_u8_up2x_batch call (head_routes), an input alone its single-image call.  Inputs with transparency go to
w2xc_process_image_rgba_u8_up2x_batch, one call per size group (head_alpha_routes; a file alone is a batch of one); with --tta 1 they stay check_tta's refusal
unless --tta_alpha 1 is given."""
import argparse
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def plan_scale(ratio):
    """(iterations, shrink_ratio) exactly as main.cpp:107-114 computes them (shrink 0.0 = none)."""
    if not ratio > 0:
        raise ValueError("scale_ratio must be positive")
    it = int(math.ceil(math.log2(ratio)))        # may be NEGATIVE for ratio < 1: the reference does not clamp it (:107-108)
    shrink = 0.0
    if int(ratio) != 2.0 ** it:                   # static_cast<int>(ratio) != std::pow(2, iter)
        shrink = ratio / 2.0 ** it                # e.g. ratio 0.3 -> iter -1 -> shrink 0.6 (NOT 0.3), ratio 0.5 -> shrink 1.0
    if shrink == 1.0:
        shrink = 0.0                              # cv::resize to the same size with INTER_LINEAR is the identity
    return max(it, 0), shrink                     # the 2x loop runs max(iter, 0) times (:126)


def auto_output_name(input_file, mode, noise_level, scale_ratio):
    """main.cpp:173-189 (std::to_string(double) prints six decimals)."""
    dot = input_file.rfind(".")
    name = input_file[:dot] if dot >= 0 else input_file
    name += "(" + mode + ")"
    if "noise" in mode:
        name += "(Level" + str(noise_level) + ")"
    if "scale" in mode:
        name += "(x" + "%.6f" % scale_ratio + ")"
    return name + ".png"


def group_inputs(files_with_sizes, mode, noise_level, scale_ratio):
    """[(file, (width, height)), ...] -> [((width, height), [files], [output names]), ...]: one entry per image size in order of first appearance, the files
    of a size in the order given; every output under its automatic name.  Pure: no file is opened."""
    groups = {}
    for name, size in files_with_sizes:
        groups.setdefault(tuple(size), []).append(name)
    return [(size, names, [auto_output_name(f, mode, noise_level, scale_ratio) for f in names]) for size, names in groups.items()]


def model_route(noise, scale):
    """'rgb' when the loaded models take three planes (w2xc_process_image_rgb_u8*), 'y' when they take one; models of different kinds, or of neither
    kind, are a SystemExit with a message.  `noise` / `scale`: (name, input planes of the first layer) or None."""
    loaded = [m for m in (noise, scale) if m is not None]
    kinds = {3: "rgb", 1: "y"}
    for name, nin in loaded:
        if nin not in kinds:
            raise SystemExit("%s: the first layer takes %d planes; only Y models (1 plane) and RGB models (3 planes) are supported" % (name, nin))
    routes = {kinds[nin] for _, nin in loaded}
    if len(routes) > 1:
        raise SystemExit("mixed model kinds: " + ", ".join("%s takes %d plane%s" % (name, nin, "" if nin == 1 else "s") for name, nin in loaded) +
                         "; use a noise model and a scale model of the same kind")
    return routes.pop() if routes else "y"


def group_alpha(files_with_sizes, mode, noise_level, scale_ratio):
    """The inputs that take the RGBA call, [(file, (width, height)), ...] -> ([files of the single calls], [[files of a batch call], ...]): group_inputs'
    groups; a group of two or more is one batch call, a file alone with its size stays the single call.  Pure: no file is opened."""
    groups = [files for _, files, _ in group_inputs(files_with_sizes, mode, noise_level, scale_ratio)]
    return [g[0] for g in groups if len(g) == 1], [g for g in groups if len(g) > 1]


def wants_alpha(arr):
    """The alpha decision, on the decoded array: True for an h x w x 4 uint8 array with at least one alpha byte below 255 (the RGBA call), False for
    everything else -- three channels, or an alpha that is 255 everywhere (the 3-channel route, as before)."""
    return arr.ndim == 3 and arr.shape[2] == 4 and bool((arr[:, :, 3] < 255).any())


def check_tta(tta, alpha_files, tta_alpha=0):
    """--tta 1 with inputs that take the RGBA call (`alpha_files`: their names) and without --tta_alpha 1: a SystemExit with a message; everything else passes"""
    if tta and alpha_files and not tta_alpha:
        raise SystemExit("--tta 1 is not applied to images with transparency (%s) by default: alpha would go through 8 variants per pass too; add "
                         "--tta_alpha 1 to run them through the TTA form of the RGBA call, convert them with --tta 0 or flatten the alpha channel first"
                         % ", ".join(alpha_files))


def alpha_tta_routes(head, alpha_groups):
    """How the inputs with transparency run under --tta 1 --tta_alpha 1: [(call, [files]), ...], ONE call per size group (`alpha_groups`: lists of names, one
    per image size) in the order given, a file alone a batch of one -- call = "rgba_up2x_batch_tta" for an upconv scale model (head_alpha_routes' grouping),
    "rgba_batch_tta" for Y and RGB models.  Pure: no file is opened."""
    if head:
        return [(call + "_tta", files) for call, files in head_alpha_routes(alpha_groups)]
    return [("rgba_batch_tta", list(g)) for g in alpha_groups if g]


def check_head(head, tta, alpha_files, groups):
    """What a scale model with an upconv head (upconv_7: the model enlarges by itself) cannot run THROUGH THE SINGLE-IMAGE RGB CALL: --tta 1, inputs that
    take the RGBA call (`alpha_files`: their names) and inputs of one size that would go as a batch (`groups`: lists of names, one per image size) are a
    SystemExit with a message, before anything is converted; everything else passes.  main hands it the transparency case alone: same-size groups and
    --tta 1 go to the head batch call (head_routes)."""
    if not head:
        return
    if tta:
        raise SystemExit("--tta 1 is not available for an upconv scale model: its TTA form is not built; use --tta 0")
    if alpha_files:
        raise SystemExit("images with transparency (%s) are not available for an upconv scale model: its RGBA form is not built; flatten the alpha "
                         "channel first" % ", ".join(alpha_files))
    batched = [g for g in groups if len(g) > 1]
    if batched:
        raise SystemExit("several inputs of one size (%s) would run as a batch, which is not built for an upconv scale model: convert them one per call"
                         % "; ".join(", ".join(g) for g in batched))


def head_routes(tta, alpha_files, groups):
    """How the opaque inputs of an upconv scale model run: [(call, [files]), ...], one entry per size group in the order given -- call = "up2x_batch" (ONE
    w2xc_process_image_rgb_u8_up2x_batch call, with tta as given) for a group of two or more files and, under --tta 1, for every group; "single" (the
    single-image RGB call) for a file alone without TTA.  Inputs with transparency (`alpha_files`) are check_head's SystemExit.  Pure: no file is opened."""
    check_head(True, 0, alpha_files, [])
    return [("up2x_batch" if tta or len(g) > 1 else "single", list(g)) for g in groups if g]


def head_alpha_routes(alpha_groups):
    """How the inputs with transparency of an upconv scale model run: [("rgba_up2x_batch", [files]), ...], ONE w2xc_process_image_rgba_u8_up2x_batch call per
    size group (`alpha_groups`: lists of names, one per image size) in the order given -- a file alone is a batch of one.  Pure: no file is opened.
    (--tta 1 never gets here: check_tta, or with --tta_alpha 1 alpha_tta_routes.)"""
    return [("rgba_up2x_batch", list(g)) for g in alpha_groups if g]


def check_inputs(ap, args):
    """-o names ONE output file: with several inputs it is refused (argparse's error exit, status 2)"""
    if len(args.input_file) > 1 and args.output_file != "(auto)":
        ap.error("-o/--output_file needs a single input file (%d given): several inputs are written under their automatic names" % len(args.input_file))
    return args


def build_parser():
    ap = argparse.ArgumentParser(description="waifu2x reimplementation using libw2xc_hip (MI355X)")
    ap.add_argument("-i", "--input_file", required=True, nargs="+", action="extend",
                    help="path to input image file (you should input full path); several files = batches of same-size images")
    ap.add_argument("-o", "--output_file", default="(auto)", help="path to output image file (you should input full path)")
    ap.add_argument("-m", "--mode", default="noise_scale", choices=["noise", "scale", "noise_scale"], help="image processing mode")
    ap.add_argument("--noise_level", type=int, default=1, choices=[1, 2], help="noise reduction level")
    ap.add_argument("--scale_ratio", type=float, default=2.0, help="custom scale ratio")
    ap.add_argument("--model_dir", default="models", help="path to custom model directory (don't append last / )")
    ap.add_argument("-j", "--jobs", type=int, default=4, help="number of threads launching at the same time")
    # not a reference flag: w2xc_opts.precision of the engine (fp32 = the reference's arithmetic on the fp32 MFMA)
    ap.add_argument("--precision", default="fp32", choices=["fp32", "bf16x3", "fp16x2", "bf16x2", "bf16"],
                    help="engine arithmetic for the CNN layers (extension; default fp32)")
    # not a reference flag in v1: later upstream versions have it as --tta
    ap.add_argument("-t", "--tta", type=int, default=0, choices=[0, 1], help="test-time augmentation: 8 flips / transposes per model pass, averaged (extension; 8x the time)")
    ap.add_argument("--tta_alpha", type=int, default=0, choices=[0, 1],
                    help="with --tta 1: also run images with transparency, colour and alpha, through test-time augmentation (extension; default 0 = refuse them)")
    return ap


def main(argv=None):
    ap = build_parser()
    args = check_inputs(ap, ap.parse_args(argv))
    from PIL import Image
    import __graft_entry__ as graft
    w2xc = graft.load_package()

    w2xc.modelUtility.getInstance().setNumberOfJobs(args.jobs)        # :79

    noise = scale = None
    noise_name, scale_name = "noise%d_model.json" % args.noise_level, "scale2.0x_model.json"
    if args.mode in ("noise", "noise_scale"):                         # :83-89
        noise = w2xc._ModelSet.from_json(os.path.join(args.model_dir, noise_name))
    iterations, shrink = 0, 0.0
    if args.mode in ("scale", "noise_scale"):                         # :103-121
        iterations, shrink = plan_scale(args.scale_ratio)
        scale = w2xc._ModelSet.from_json(os.path.join(args.model_dir, scale_name))
        print("start scaling")
    rgb = model_route((noise_name, noise.planes(0)[0]) if noise else None, (scale_name, scale.planes(0)[0]) if scale else None) == "rgb"
    process, process_batch = (w2xc.process_image_rgb_u8, w2xc.process_image_rgb_u8_batch) if rgb else (w2xc.process_image_u8, w2xc.process_image_u8_batch)

    def load(path):
        pil = Image.open(path)
        if pil.mode in ("RGBA", "LA", "PA", "RGBa", "La") or "transparency" in pil.info:
            im = np.asarray(pil.convert("RGBA"))
            if wants_alpha(im):
                return np.ascontiguousarray(im if rgb else im[:, :, [2, 1, 0, 3]])   # (the colour order of the route, alpha last)
        im = np.asarray(pil.convert("RGB"))
        return np.ascontiguousarray(im if rgb else im[:, :, ::-1])   # Y route: cv::imread(IMREAD_COLOR)'s BGR order (Q3); RGB models take RGB as it is
    images = [load(f) for f in args.input_file]
    opaque = [(f, im) for f, im in zip(args.input_file, images) if im.shape[2] == 3]
    check_tta(args.tta, [f for f, im in zip(args.input_file, images) if im.shape[2] == 4], args.tta_alpha)
    head = bool(scale is not None and iterations and scale.has_head)   # (an upconv model: the RGB route's single-image call, passed through as it is)
    # (the transparent inputs of a head model have a call of their own, head_alpha_routes below: head_routes sees the opaque ones alone)
    routes = head_routes(args.tta, [],
                         [files for _, files, _ in group_inputs([(f, (im.shape[1], im.shape[0])) for f, im in opaque], args.mode, args.noise_level,
                                                                args.scale_ratio)]) if head else []
    tta = dict(tta=True) if args.tta else {}
    outs = {}
    if noise is None and iterations == 0 and not shrink:
        outs = dict(zip(args.input_file, images))                      # ratio 1.0 in scale mode: nothing to do
    elif iterations == 0 and noise is None:
        raise SystemExit("scale_ratio %g needs no 2x step; the reference would only shrink, which is not supported without a model pass" % args.scale_ratio)
    else:
        prec = {"fp32": w2xc.PRECISION_FP32, "bf16": w2xc.PRECISION_BF16, "bf16x2": w2xc.PRECISION_BF16X2, "bf16x3": w2xc.PRECISION_BF16X3, "fp16x2": w2xc.PRECISION_FP16X2}[args.precision]
        opts = w2xc.make_opts(precision=prec)      # always explicit: an explicit --precision beats the W2XC_PRECISION env default
        alpha = {f: im for f, im in zip(args.input_file, images) if im.shape[2] == 4}
        alpha_sized = [(f, (im.shape[1], im.shape[0])) for f, im in alpha.items()]
        alpha_groups = [files for _, files, _ in group_inputs(alpha_sized, args.mode, args.noise_level, args.scale_ratio)]
        singles, batches = ([], []) if head or args.tta else group_alpha(alpha_sized, args.mode, args.noise_level, args.scale_ratio)
        if args.tta:   # (--tta_alpha 1, or there are no such inputs -- check_tta: the TTA form of the RGBA call of the models, one call per size group)
            for call, files in alpha_tta_routes(head, alpha_groups):
                fn = w2xc.process_image_rgba_u8_up2x_batch if call == "rgba_up2x_batch_tta" else w2xc.process_image_rgba_u8_batch
                outs.update(zip(files, fn([alpha[f] for f in files], noise, scale if iterations else None, iterations, opts, shrink, tta=True)))
        elif head:   # (an upconv scale model: the RGBA head call per size group)
            for _, files in head_alpha_routes([files for _, files, _ in group_inputs(alpha_sized, args.mode, args.noise_level, args.scale_ratio)]):
                outs.update(zip(files, w2xc.process_image_rgba_u8_up2x_batch([alpha[f] for f in files], noise, scale, iterations, opts, shrink)))
        for f in singles:
            outs[f] = w2xc.process_image_rgba_u8(alpha[f], noise, scale if iterations else None, iterations, opts, shrink)
        for files in batches:                      # one batch call per image size
            outs.update(zip(files, w2xc.process_image_rgba_u8_batch([alpha[f] for f in files], noise, scale if iterations else None, iterations, opts, shrink)))
        if head:   # (an upconv scale model: the head batch call per size group, an input alone its single-image call -- head_routes)
            by_file = dict(opaque)
            for call, files in routes:
                if call == "single":
                    outs[files[0]] = process(by_file[files[0]], noise, scale, iterations, opts, shrink)
                else:
                    outs.update(zip(files, w2xc.process_image_rgb_u8_up2x_batch([by_file[f] for f in files], noise, scale, iterations, opts, shrink, **tta)))
        elif len(opaque) == 1:
            for f, im in opaque:
                outs[f] = process(im, noise, scale if iterations else None, iterations, opts, shrink, **tta)
        elif opaque:
            by_file = dict(opaque)
            sized = [(f, (im.shape[1], im.shape[0])) for f, im in opaque]
            for _, files, _ in group_inputs(sized, args.mode, args.noise_level, args.scale_ratio):   # one batch call per image size
                res = process_batch([by_file[f] for f in files], noise, scale if iterations else None, iterations, opts, shrink, **tta)
                outs.update(zip(files, res))
    for f in args.input_file:
        name = args.output_file
        if name == "(auto)":
            name = auto_output_name(f, args.mode, args.noise_level, args.scale_ratio)
        res = outs[f]
        if not rgb:
            res = res[:, :, ::-1] if res.shape[2] == 3 else res[:, :, [2, 1, 0, 3]]
        Image.fromarray(np.ascontiguousarray(res)).save(name)
    print("process successfully done!")
    return 0


if __name__ == "__main__":
    sys.exit(main())
