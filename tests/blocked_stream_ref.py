"""The case list of the version 2 stream tests (the container's CPU restatement itself is oracle/blocked_stream.py)."""
import numpy as np


def small_cases(oracle):
    """The shape list of tests/test_gpu_blocked.py::test_stagewise_small plus the option cases of the issue: (name, img, alpha, oracle keywords)."""
    out = []
    for kind, alpha, shape in (("pn", True, (256, 128)), ("rg", True, (256, 128)), ("rga", True, (203, 61)), ("pn", False, (131, 77)), ("rg", False, (64, 64)),
                               ("pn", True, (8, 8)), ("pn", True, (9, 9)), ("rg", False, (17, 10)), ("pn", True, (1, 1)), ("pn", True, (2, 65)), ("pn", False, (25, 33)),
                               ("rg", True, (265, 9)), ("flat", True, (96, 80)), ("flat", True, (200, 168))):
        w, h = shape
        if kind == "flat":
            img = np.full((h, w), 0xFF336699, dtype=np.uint32)
        elif kind == "pn":
            img = oracle.photo_noise(w, h, 5)
        else:
            img = oracle.random_gradient(w, h, 5, kind == "rg")
        out.append(("%s-%dx%d-%s" % (kind, w, h, "rgba" if alpha else "rgb"), img, alpha, {}))
    rga = oracle.random_gradient(128, 64, 3, False)
    for ef in (0, 25, 400):
        out.append(("rga-ef%d" % ef, rga, True, dict(error_factor=ef)))
    out.append(("rga-accurate", rga, True, dict(fast=False)))
    out.append(("pn-accurate-rgb", oracle.photo_noise(72, 40, 7), False, dict(fast=False)))
    out.append(("rga-pcg", rga, True, dict(dither_mode=1)))
    out.append(("pn-pcg-ragged", oracle.photo_noise(75, 41, 7), True, dict(dither_mode=1)))
    for shift in ((8, 8, 8), (0, 0, 0), (3, 5, 8)):
        out.append(("rga-forced%d%d%d" % shift, rga, True, dict(forced_shift=shift)))
    out.append(("rga-ragged-forced888", oracle.random_gradient(75, 41, 3, False), True, dict(forced_shift=(8, 8, 8))))
    ramp = np.zeros((64, 512), dtype=np.uint32)
    ramp[:] = 0xFF000000 | (np.arange(512, dtype=np.uint32)[None, :] // 4) * 0x010101  # a slow horizontal ramp: one very wide rectangle
    out.append(("ramp", ramp, True, {}))
    return out


def stream_flags(kw):
    return (1 if kw.get("fast", True) else 0) | (2 if kw.get("dither_mode", 0) else 0)
