"""Writes tests/golden/caseG_resample.npz with Pillow: for every case of tests/resample_refs.py (GOLDEN_CASES x RGB / RGBA) the input bytes and what
`Image.fromarray(img).resize((W', H'), Image.LANCZOS | Image.BILINEAR)` returns for them, plus the Pillow version.  Random bytes, about 150 KB.

      python tests/gen_golden_resample.py [--check]     (--check: regenerate and compare byte for byte)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def pillow_resize(img, out_hw, name):
    from PIL import Image
    flt = {"lanczos": Image.LANCZOS, "bilinear": Image.BILINEAR}[name]
    return np.asarray(Image.fromarray(img).resize((out_hw[1], out_hw[0]), flt))


def generate():
    import PIL
    from tests import resample_refs as R
    out = {"pillow_version": np.array(PIL.__version__)}
    for hw, out_hw in R.GOLDEN_CASES:
        for C in (3, 4):
            name = R.case_name(hw, out_hw, C)
            img = R.case_image(hw, C)
            out["in_" + name] = img
            for flt in R.FILTERS:
                out[f"{flt}_{name}"] = pillow_resize(img, out_hw, flt)
    return out


if __name__ == "__main__":
    from tests import resample_refs as R
    out = generate()
    if "--check" in sys.argv:
        z = np.load(R.GOLDEN)
        assert sorted(z.files) == sorted(out), (z.files, sorted(out))
        for k in out:
            assert np.array_equal(z[k], out[k]), k
        print("golden matches byte for byte:", R.GOLDEN)
    else:
        np.savez_compressed(R.GOLDEN, **out)
        print("wrote", R.GOLDEN, os.path.getsize(R.GOLDEN), "bytes")
