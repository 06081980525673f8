"""Image-folder trees written at test time (test infrastructure only): an ImageNet-style class-per-directory
tree, TinyImageNet in both of its forms, and a decoder that needs no Pillow. Nothing here comes from a published
dataset: every pixel is drawn from a seeded generator."""
import os
import zlib

import numpy as np


def pixels(h, w, seed):
    """uint8 [h, w, 3]: smooth ramps plus noise, so that a JPEG of it is not flat"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([(yy * 255 // max(1, h - 1)), (xx * 255 // max(1, w - 1)), ((yy + xx) * 7 % 256)], -1)
    return ((base + rng.integers(0, 64, (h, w, 3))) % 256).astype(np.uint8)


def save_image(path, array, **kw):
    """write `array` (uint8 [h, w, 3] or [h, w]) with Pillow; the format follows the extension"""
    from PIL import Image
    os.makedirs(os.path.dirname(path), exist_ok=True)
    ext = os.path.splitext(path)[1].lower()
    fmt = {".jpeg": "JPEG", ".jpg": "JPEG", ".png": "PNG", ".bmp": "BMP"}[ext]
    Image.fromarray(array).save(path, format=fmt, **kw)


def touch(path, data=b""):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "wb") as f:
        f.write(data)


def write_image_folder(root, per_class=4, classes=("n03", "n01", "n02"), seed=0, sizes=None):
    """root/<class>/<files>: `per_class` PNG and JPEG files of mixed sizes per class, the class directories
    created in the order given (not sorted). Returns {path: uint8 array as written}."""
    sizes = sizes or [(24, 31), (40, 17), (9, 50), (33, 33), (64, 48), (12, 12)]
    written = {}
    k = 0
    for cls in classes:
        for i in range(per_class):
            h, w = sizes[k % len(sizes)]
            ext = ".png" if k % 2 == 0 else ".JPEG"
            path = os.path.join(root, cls, f"img_{i}{ext}")
            a = pixels(h, w, seed * 1000 + k)
            save_image(path, a, **({} if ext == ".png" else {"quality": 90}))
            written[path] = a
            k += 1
    return written


def write_tiny_imagenet(root, classes=("n30", "n10", "n20"), per_class=4, n_val=6, seed=0, val_form="folders"):
    """root/train/<class>/images/<class>_<i>.JPEG (64 x 64, as published; a few other sizes mixed in) and
    root/val in `val_form`: 'folders' (val/<class>/images/...) or 'annotations' (val/images/val_<i>.JPEG +
    val/val_annotations.txt, the published download). Returns (train [(path, class)], val [(path, class)])."""
    train, val = [], []
    k = 0
    for cls in classes:
        for i in range(per_class):
            h, w = [(64, 64), (64, 64), (48, 64), (70, 30)][k % 4]
            path = os.path.join(root, "train", cls, "images", f"{cls}_{i}.JPEG")
            save_image(path, pixels(h, w, seed * 1000 + k), quality=90)
            train.append((path, cls))
            k += 1
        touch(os.path.join(root, "train", cls, f"{cls}_boxes.txt"), b"not an image\n")
    lines = []
    for i in range(n_val):
        cls = classes[(i * 2 + 1) % len(classes)]
        if val_form == "folders":
            path = os.path.join(root, "val", cls, "images", f"val_{i}.JPEG")
        else:
            path = os.path.join(root, "val", "images", f"val_{i}.JPEG")
            lines.append(f"val_{i}.JPEG\t{cls}\t0\t0\t10\t10\n")
        save_image(path, pixels(64, 64, seed * 1000 + 500 + i), quality=90)
        val.append((path, cls))
    if val_form != "folders":
        touch(os.path.join(root, "val", "val_annotations.txt"), "".join(lines).encode())
    return train, val


def fake_decode(path):
    """a deterministic uint8 image of a path-dependent size between 3 x 5 and 40 x 70, with no file and no
    Pillow behind it: for the loader's mechanics"""
    seed = zlib.crc32(os.fsencode(path))
    h, w = 3 + seed % 38, 5 + (seed // 64) % 66
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)
