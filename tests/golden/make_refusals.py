"""Generate tests/golden/image_call_refusals.json: what every entry point of the image, RGBA, YUV-frame and TTA-block families answers to a
call with TWO independent things wrong at once -- (entry, case, return code, w2xc_last_error() text).  The order in which an entry point
checks its arguments decides which of the two it names; tests/test_image_refusals.py replays every recorded case against the built library
and compares code and text exactly, so a change of that order shows.

Run on a machine WITHOUT a HIP device, from the commit whose behaviour is to be pinned:  python tests/golden/make_refusals.py
(every recorded call is refused before a device is touched; a call that gets as far as asking for one answers W2XC_ERR_HIP there, depends
on the machine and is dropped.  With a device such a call would run on the made-up pointers below: the generator refuses to start.)

tests/test_image_refusals.py imports cases() from here: the calls are written once."""
import ctypes as C
import itertools
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "image_call_refusals.json")

# made-up addresses, never read or written: every recorded call is refused on its arguments
A_IN, A_OUT, A_UP, A_TR = 0x10000000, 0x20000000, 0x30000000, 0x40000000
W, H = 6, 4


def models(w2xc):
    """tiny models with constant weights: a Y model, an RGB model, an upconv head model (three planes)"""
    def layers(planes):
        return [(i, o, np.full((o, i, 3, 3), 0.01, np.float32), np.zeros(o)) for i, o in zip(planes[:-1], planes[1:])]
    return {"y": w2xc._ModelSet.from_layers(layers([1, 32, 1])), "rgb": w2xc._ModelSet.from_layers(layers([3, 32, 3])),
            "head": w2xc._ModelSet.from_layers(layers([3, 32, 32]), head=(np.full((32, 3, 4, 4), 0.01, np.float32), None))}


class Side(dict):
    """one w2xc_yuv_planes argument as a dict of its fields"""


def _side(w, h, cw, ch, at):
    return Side(y=at, y_stride=w, y_frame_stride=w * h, u=at + 0x100000, v=at + 0x200000, c_stride=cw, c_frame_stride=cw * ch, c_px=1)


def _marshal(w2xc, v, keep):
    """a case's value -> the ctypes argument (keep: what must outlive the call)"""
    if isinstance(v, Side):
        s = w2xc.YuvPlanes(**v)
        keep.append(s)
        return C.byref(s)
    if isinstance(v, list):   # the image pointers of a host batch
        a = (C.c_void_p * max(len(v), 1))(*v)
        keep.append(a)
        return a
    if isinstance(v, float):
        return C.c_double(v)
    return v


def _set(args, key, value):
    """args with `key` replaced; "in.c_px" = field c_px of the Side `in`"""
    if "." in key:
        name, field = key.split(".")
        side = Side(args[name])
        side[field] = value
        args[name] = side
    else:
        args[key] = value


def _entries(M):
    """(entry, ordered base arguments of a valid call, {fault: {argument: value}}) of every entry point"""
    y, rgb, head = M["y"].handle, M["rgb"].handle, M["head"].handle
    out = []

    # ---- the image and RGBA calls: single / batch, device / host ----
    def image(name, px, model, batch=False, host=False, shrink=True, bleed=False, tta=False, noise=True, up2x=False):
        a = {}
        if noise:
            a["noise"] = None
        a["scale"] = model
        if batch:
            a["n"] = 2
        a["in"] = [A_IN, A_IN + 0x1000] if batch and host else A_IN
        if batch and not host:
            a["in_img"] = W * px * H
        a["in_stride"] = W * px
        a["w"], a["h"] = W, H
        a["out"] = [A_OUT, A_OUT + 0x1000] if batch and host else A_OUT
        if batch and not host:
            a["out_img"] = 2 * W * px * 2 * H
        a["out_stride"] = 2 * W * px
        a["iterations"] = 1
        if shrink:
            a["shrink"] = 0.0
        if bleed:
            a["bleed"] = -1
        if not host:
            a["stream"] = None
        a["opts"] = None
        if tta:
            a["tta"] = 0
        f = {"null_in": {"in": None}, "null_out": {"out": None}, "in_stride_short": {"in_stride": W * px - 1}, "out_stride_short": {"out_stride": 2 * W * px - 1},
             "iterations_5": {"iterations": 5}, "no_model": {"scale": None}, "w_0": {"w": 0}}
        f["overlap"] = {"out": a["in"]}
        if batch:
            f["n_0"] = {"n": 0}
            if not host:
                f["out_img_short"] = {"out_img": 1}
        if shrink:
            f["shrink_1"] = {"shrink": 1.0}
        if tta:
            f["tta_2"] = {"tta": 2}
        if noise:
            f["head_noise"] = {"noise": head}
            f["y_beside_rgb"] = {"noise": y, "scale": rgb} if model != y else {"noise": rgb, "scale": y}
            f["rgb_beside_y"] = {"noise": rgb, "scale": y} if model != y else {"noise": y, "scale": rgb}
        f["wrong_scale"] = {"scale": rgb if up2x else head}   # (a head model where it is refused; no head model where one is asked)
        f["other_route"] = {"scale": rgb if model == y else y}
        out.append((name, a, f))

    for fam, px, model in (("w2xc_process_image_u8", 3, y), ("w2xc_process_image_rgb_u8", 3, rgb)):
        image(fam + "_tta_device", px, model, tta=True)
        image(fam + "_ex_device", px, model)
        image(fam + "_tta", px, model, host=True, tta=True)
        image(fam + "_ex", px, model, host=True)
        image(fam + "_batch_tta_device", px, model, batch=True, tta=True)
        image(fam + "_batch_device", px, model, batch=True)
        image(fam + "_batch_tta", px, model, batch=True, host=True, tta=True)
        image(fam + "_batch", px, model, batch=True, host=True)
    image("w2xc_process_image_u8_device", 3, y, shrink=False)
    image("w2xc_process_image_u8", 3, y, host=True, shrink=False)
    image("w2xc_scale2x_image_u8_device", 3, y, shrink=False, noise=False)
    image("w2xc_scale2x_image_u8", 3, y, host=True, shrink=False, noise=False)
    image("w2xc_process_image_rgb_u8_up2x_batch_device", 3, head, batch=True, tta=True, up2x=True)
    image("w2xc_process_image_rgb_u8_up2x_batch", 3, head, batch=True, host=True, tta=True, up2x=True)
    for route, model in (("", y), ("#rgb", rgb)):   # (the models choose the route: both)
        image("w2xc_process_image_rgba_u8_ex_device" + route, 4, model, bleed=True)
        image("w2xc_process_image_rgba_u8_ex" + route, 4, model, host=True, bleed=True)
        image("w2xc_process_image_rgba_u8_batch_tta_device" + route, 4, model, batch=True, bleed=True, tta=True)
        image("w2xc_process_image_rgba_u8_batch_device" + route, 4, model, batch=True, bleed=True)
        image("w2xc_process_image_rgba_u8_batch_tta" + route, 4, model, batch=True, host=True, bleed=True, tta=True)
        image("w2xc_process_image_rgba_u8_batch" + route, 4, model, batch=True, host=True, bleed=True)
    image("w2xc_process_image_rgba_u8_up2x_batch_tta_device", 4, head, batch=True, bleed=True, tta=True, up2x=True)
    image("w2xc_process_image_rgba_u8_up2x_batch_device", 4, head, batch=True, bleed=True, up2x=True)
    image("w2xc_process_image_rgba_u8_up2x_batch_tta", 4, head, batch=True, host=True, bleed=True, tta=True, up2x=True)
    image("w2xc_process_image_rgba_u8_up2x_batch", 4, head, batch=True, host=True, bleed=True, up2x=True)

    # ---- YUV frames ----
    cw, ch = (W + 1) // 2, (H + 1) // 2
    for name, model, host in (("w2xc_process_frames_yuv_u8_device", y, False), ("w2xc_process_frames_yuv_u8", y, True),
                              ("w2xc_process_frames_yuv_u8_rgb_device", rgb, False), ("w2xc_process_frames_yuv_u8_rgb", rgb, True)):
        is_rgb = model == rgb
        a = {"noise": None, "scale": model, "n": 2, "w": W, "h": H, "chroma": 0, "range": 1}
        if is_rgb:
            a["matrix"] = 1
        a["in"], a["out"] = _side(W, H, cw, ch, A_IN), _side(2 * W, 2 * H, 2 * cw, 2 * ch, A_OUT)
        a["iterations"] = 1
        if not host:
            a["stream"] = None
        a["opts"] = None
        f = {"null_in": {"in": None}, "null_out_y": {"out.y": None}, "null_in_u": {"in.u": None}, "n_0": {"n": 0}, "y_stride_short": {"in.y_stride": W - 1},
             "c_stride_short": {"out.c_stride": 2 * cw - 1}, "overlap": {"out.y": A_IN}, "iterations_2": {"iterations": 2}, "no_model": {"scale": None},
             "head_noise": {"noise": head}, "wrong_scale": {"scale": rgb if not is_rgb else y},
             "y_beside_rgb": {"noise": y, "scale": rgb} if is_rgb else {"noise": rgb, "scale": y}, "chroma_7": {"chroma": 7}, "chroma_400": {"chroma": 3},
             "range_5": {"range": 5}, "c_px_3": {"in.c_px": 3}, "w_0": {"w": 0}}
        if is_rgb:
            f["matrix_9"] = {"matrix": 9}
        else:
            f["head_scale"] = {"scale": head}
        if host:
            f["c_px_2_apart"] = {"in.c_px": 2, "in.c_stride": 2 * cw, "in.c_frame_stride": 2 * cw * ch}   # (interleaved planes that do not interleave)
        out.append((name, a, f))

    # ---- the YUV building blocks ----
    rgb_planes = {"rgb": A_OUT, "image_stride": 3 * 4 * W * H, "plane_stride": 4 * W * H}
    yuv_f = {"null_side": {"side": None}, "null_rgb": {"rgb": None}, "null_y": {"side.y": None}, "n_0": {"n": 0}, "y_stride_short": {"side.y_stride": W - 1},
             "plane_stride_short": {"plane_stride": 4 * W * H - 4}, "plane_stride_odd": {"plane_stride": 4 * W * H + 2}, "overlap": {"rgb": A_IN},
             "chroma_7": {"chroma": 7}, "chroma_400": {"chroma": 3}, "range_5": {"range": 5}, "matrix_9": {"matrix": 9}, "c_px_3": {"side.c_px": 3}, "w_0": {"w": 0}}
    geom = {"n": 2, "w": W, "h": H, "chroma": 0, "range": 1, "matrix": 1}
    out.append(("w2xc_yuv8_to_rgb_device", dict(side=_side(W, H, cw, ch, A_IN), **geom, **rgb_planes, stream=None), yuv_f))
    out.append(("w2xc_rgb_to_yuv8_device", dict(**rgb_planes, **geom, side=_side(W, H, cw, ch, A_IN), stream=None), yuv_f))
    y8_f = {"null_bytes": {"bytes": None}, "null_plane": {"plane": None}, "n_0": {"n": 0}, "stride_short": {"stride": W - 1}, "frame_stride_short": {"frame_stride": 1},
            "plane_stride_odd": {"plane_stride": 4 * W * H + 2}, "overlap": {"plane": A_IN}, "range_5": {"range": 5}, "w_0": {"w": 0}}
    out.append(("w2xc_y8_to_plane_device", dict(bytes=A_IN, n=2, frame_stride=W * H, stride=W, w=W, h=H, range=1, plane=A_OUT, plane_stride=4 * W * H, stream=None), y8_f))
    out.append(("w2xc_plane_to_y8_device", dict(plane=A_OUT, n=2, plane_stride=4 * W * H, w=W, h=H, range=1, bytes=A_IN, frame_stride=W * H, stride=W, stream=None), y8_f))
    out.append(("w2xc_chroma2x_u8_device",
                dict(src=A_IN, n=2, src_frame_stride=cw * ch, src_stride=cw, src_px=1, cw=cw, ch=ch, dst=A_OUT, dst_frame_stride=4 * cw * ch, dst_stride=2 * cw, dst_px=1,
                     ow=2 * cw, oh=2 * ch, stream=None),
                {"null_src": {"src": None}, "null_dst": {"dst": None}, "n_0": {"n": 0}, "src_stride_short": {"src_stride": cw - 1}, "dst_stride_short": {"dst_stride": 2 * cw - 1},
                 "overlap": {"dst": A_IN}, "src_px_3": {"src_px": 3}, "dst_px_3": {"dst_px": 3}, "ow_large": {"ow": 2 * cw + 1}, "cw_0": {"cw": 0}}))

    # ---- test-time augmentation: the plane calls and the building blocks ----
    for name, model in (("w2xc_convert_batch_tta_device", y), ("w2xc_convert_planes_tta_device", rgb)):
        k = 1 if model == y else 3   # (the second argument: planes of the batch / input planes of the model)
        a = dict(m=model, n=k, nn2x=0, src=A_IN, in_plane_stride=4 * W * H, in_stride=4 * W, w=W, h=H, dst=A_OUT, out_plane_stride=4 * W * H, out_stride=4 * W,
                 stream=None, opts=None)
        out.append((name, a, {"null_in": {"src": None}, "null_out": {"dst": None}, "null_model": {"m": None}, "n_0": {"n": 0}, "nn2x_2": {"nn2x": 2},
                              "in_stride_short": {"in_stride": 4 * W - 4}, "out_stride_odd": {"out_stride": 4 * W + 2}, "overlap": {"dst": A_IN},
                              "head_model": {"m": head}, "other_planes": {"m": rgb if model == y else y}, "w_0": {"w": 0}}))
    var = 4 * W * H
    tta_f = {"null_planes": {"planes": None}, "null_up": {"up": None}, "null_tr": {"tr": None}, "n_0": {"n": 0}, "stride_short": {"stride": 4 * W - 4},
             "stride_odd": {"stride": 4 * W + 2}, "variant_short": {"variant": var - 4}, "overlap": {"up": A_IN}, "groups_overlap": {"tr": A_UP}, "w_0": {"w": 0}}
    out.append(("w2xc_tta_spread_device", dict(planes=A_IN, n=2, plane_stride=var, stride=4 * W, w=W, h=H, up=A_UP, tr=A_TR, variant=var, stream=None), tta_f))
    out.append(("w2xc_tta_gather_device", dict(up=A_UP, tr=A_TR, variant=var, n=2, w=W, h=H, planes=A_IN, plane_stride=var, stride=4 * W, stream=None), tta_f))
    u8_f = {"null_images": {"images": None}, "null_up": {"up": None}, "n_0": {"n": 0}, "stride_short": {"stride": 3 * W - 1}, "image_stride_short": {"image_stride": 1},
            "px_5": {"px": 5}, "variant_odd": {"variant": var + 2}, "variant_short": {"variant": var - 4}, "overlap": {"up": A_IN}, "w_0": {"w": 0}}
    out.append(("w2xc_tta_spread_u8_device", dict(images=A_IN, n=2, image_stride=3 * W * H, stride=3 * W, px=3, ch0=0, ch_step=1, w=W, h=H, up=A_UP, tr=A_TR, variant=var,
                                                  stream=None), dict(u8_f, ch0_3={"ch0": 3}, ch_step_neg={"ch_step": -1})))
    out.append(("w2xc_tta_gather_u8_device", dict(up=A_UP, tr=A_TR, variant=var, n=2, planes_per_image=3, first_plane=0, n_ch=3, w=W, h=H, images=A_IN, image_stride=3 * W * H,
                                                  stride=3 * W, px=3, byte0=0, stream=None),
                dict(u8_f, planes_0={"planes_per_image": 0}, byte0_1={"byte0": 1}, first_plane_1={"first_plane": 1}, n_ch_0={"n_ch": 0})))

    # ---- the bleed, the colour and the resize blocks of the image unit ----
    out.append(("w2xc_bleed_rgba_u8_device", dict(src=A_IN, in_stride=4 * W, w=W, h=H, passes=2, dst=A_OUT, out_stride=3 * W, stream=None),
                {"null_in": {"src": None}, "null_out": {"dst": None}, "in_stride_short": {"in_stride": 4 * W - 1}, "out_stride_short": {"out_stride": 3 * W - 1},
                 "passes_neg": {"passes": -1}, "overlap": {"dst": A_IN}, "w_0": {"w": 0}}))
    img_f = {"null_image": {"image": None}, "null_plane": {"c1": None}, "stride_short": {"stride": 3 * W - 1}, "w_0": {"w": 0}, "h_0": {"h": 0}}
    for kind in ("yuv", "rgb"):
        out.append(("w2xc_u8_to_%s_device" % kind, dict(image=A_IN, stride=3 * W, w=W, h=H, c0=A_OUT, c1=A_UP, c2=A_TR, stream=None), img_f))
        out.append(("w2xc_%s_to_u8_device" % kind, dict(c0=A_OUT, c1=A_UP, c2=A_TR, w=W, h=H, image=A_IN, stride=3 * W, stream=None), img_f))
    out.append(("w2xc_resize2x_cubic_device", dict(src=A_IN, w=W, h=H, dst=A_OUT, stream=None), {"null_src": {"src": None}, "null_dst": {"dst": None}, "w_0": {"w": 0}, "h_0": {"h": 0}}))
    out.append(("w2xc_resize_linear_device", dict(src=A_IN, sw=W, sh=H, dst=A_OUT, dw=W - 1, dh=H - 1, stream=None),
                {"null_src": {"src": None}, "null_dst": {"dst": None}, "sw_0": {"sw": 0}, "dh_0": {"dh": 0}}))
    return out


def cases(w2xc, M):
    """{(entry, case): call}: every pair of faults of an entry that touch different arguments; call() -> (return code, last-error text).
    entry "name#route" = the entry point `name` with the models of another route as its valid base."""
    table = {}
    for entry, base, faults in _entries(M):
        fn = getattr(w2xc.lib(), entry.split("#")[0])
        for (na, fa), (nb, fb) in itertools.combinations(sorted(faults.items()), 2):
            if {k.split(".")[0] for k in fa} & {k.split(".")[0] for k in fb}:
                continue   # (not independent: both change the same argument)

            def call(fn=fn, base=base, changes=(fa, fb)):
                args = dict(base)
                for ch in changes:
                    for k, v in ch.items():
                        _set(args, k, v)
                keep = []
                rc = fn(*[_marshal(w2xc, v, keep) for v in args.values()])
                return rc, w2xc.last_error()
            table[(entry, na + "+" + nb)] = call
    return table


FORMAT = ("first[i][k] of an entry is one call with the two faults faults[i] and faults[i + 1 + k]: the character is the index (0-9, a-z, A-Z) into answers of "
          "the [return code, last-error text] it got, '.' = not recorded. Readable rows: python tests/golden/make_refusals.py --dump")
DIGITS = "0123456789abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ"   # one character = one index into "answers"; "." = not recorded


def _pairs(faults):
    """the case names of an entry in the file's order: row i of "first" holds faults[i] + "+" + faults[j] for every j > i"""
    return [[a + "+" + b for b in faults[i + 1:]] for i, a in enumerate(faults[:-1])]


def load(path=OUT):
    """the file -> {entry: [[case, return code, last-error text], ...]}"""
    with open(path) as f:
        d = json.load(f)
    return {entry: [[case, *d["answers"][DIGITS.index(ch)]] for names, row in zip(_pairs(e["faults"]), e["first"]) for case, ch in zip(names, row) if ch != "."]
            for entry, e in d["entries"].items()}


def main():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as entry
    w2xc = entry.load_package()
    if w2xc.device_count() > 0:
        raise SystemExit("make_refusals.py runs on a machine without a HIP device (see the module's docstring)")
    M = models(w2xc)
    got, kept, dropped = {}, 0, 0
    for (name, case), call in sorted(cases(w2xc, M).items()):
        rc, text = call()
        if rc == w2xc.ERR_HIP or rc == w2xc.OK:
            dropped += 1   # (the call got as far as a device: machine-dependent)
            continue
        got[(name, case)] = (rc, text)
        kept += 1
    # the texts repeat from call to call, so the file holds each once: {"answers": [[return code, last-error text], ...],
    # "entries": {entry: {"faults": [sorted names], "first": [one string per fault but the last, one character per later fault]}}}
    answers = sorted(set(got.values()))
    assert len(answers) <= len(DIGITS)
    entries = {}
    for name, _, faults in _entries(M):
        names = sorted(faults)
        first = ["".join(DIGITS[answers.index(got[(name, c)])] if (name, c) in got else "." for c in row) for row in _pairs(names)]
        entries[name] = {"faults": names, "first": first}
    with open(OUT, "w") as f:
        f.write('{"format": %s,\n"answers": [\n' % json.dumps(FORMAT) + ",\n".join(json.dumps(a) for a in answers) + '\n],\n"entries": {\n'
                + ",\n".join("%s: %s" % (json.dumps(k), json.dumps(v)) for k, v in sorted(entries.items())) + "\n}}\n")
    print("%d refusals recorded, %d calls dropped (they reach a device)" % (kept, dropped))


if __name__ == "__main__":
    if sys.argv[1:] == ["--dump"]:   # the record as readable rows, e.g. to compare two versions of the file: entry, case, return code, text
        for name, rows in sorted(load().items()):
            for row in rows:
                print(json.dumps([name] + row))
    else:
        main()
