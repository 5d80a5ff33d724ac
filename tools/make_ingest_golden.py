"""Writes tests/golden/ingest_pil.npz: raw uint8 clips and the uint8 images PIL itself makes of them (crop, then
Image.resize(..., BILINEAR) -- what torchvision's CenterCrop / Resize run on a PIL image), for the clip-ingest tests on machines
without PIL.  Needs Pillow and numpy only.

    python tools/make_ingest_golden.py

Per geometry one clip of three frames: random bytes, random 0 / 255, a ramp.  Keys: raw:<name> uint8 [1, 3, Hin, Win, C] (kth64 and
kth128 share raw:kth), pil:<tag> uint8 [1, 3, Hout, Wout, C], meta = JSON string {tag: {raw, crop, out}, "pillow": version}."""
import json
import os

import numpy as np
import PIL
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "ingest_pil.npz")

# tag -> (raw name, Hin, Win, C, crop box (top, left, h, w) or None, (Hout, Wout)); tests/ingest_ref.py: GOLDEN_GEOMETRIES
GEOMETRIES = {
    "kth64": ("kth", 120, 160, 1, (0, 20, 120, 120), (64, 64)),
    "kth128": ("kth", 120, 160, 1, (0, 20, 120, 120), (128, 128)),
    "bair": ("bair", 64, 64, 3, None, (64, 64)),
    "odd": ("odd", 37, 53, 3, (3, 5, 31, 41), (16, 24)),
    "down4": ("down4", 240, 240, 1, None, (64, 64)),
}


def frames(H, W, C, seed):
    rs = np.random.RandomState(seed)
    y, x, c = np.meshgrid(np.arange(H), np.arange(W), np.arange(C), indexing="ij")
    return np.stack([rs.randint(0, 256, size=(H, W, C)), rs.randint(0, 2, size=(H, W, C)) * 255, (3 * x + 5 * y + 41 * c) % 256]).astype(np.uint8)


def pil_frame(f, crop, out_hw):
    img = Image.fromarray(f[:, :, 0], "L") if f.shape[2] == 1 else Image.fromarray(f, "RGB")
    if crop is not None:
        top, left, h, w = crop
        img = img.crop((left, top, left + w, top + h))
    if (img.height, img.width) != tuple(out_hw):
        img = img.resize((out_hw[1], out_hw[0]), Image.BILINEAR)
    a = np.asarray(img)
    return a[:, :, None] if a.ndim == 2 else a


def main():
    arrays, meta = {}, {"pillow": PIL.__version__}
    for i, (tag, (name, H, W, C, crop, out_hw)) in enumerate(GEOMETRIES.items()):
        if "raw:" + name not in arrays:
            arrays["raw:" + name] = frames(H, W, C, 7000 + i)[None]
        raw = arrays["raw:" + name]
        arrays["pil:" + tag] = np.stack([pil_frame(f, crop, out_hw) for f in raw[0]])[None]
        meta[tag] = {"raw": name, "crop": crop, "out": list(out_hw)}
    arrays["meta"] = np.array(json.dumps(meta))
    np.savez_compressed(OUT, **arrays)
    print("wrote %s: %d bytes" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
