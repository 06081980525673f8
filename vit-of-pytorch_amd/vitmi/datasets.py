"""CIFAR-10 / CIFAR-100 and ImageNet / TinyImageNet image folders from disk, without torchvision (host only:
no GPU, no library). CIFAR first; the image folders are at the end of this file.

The reference builds its loaders from `torchvision.datasets.CIFAR10 / CIFAR100(root=os.path.join(
config.data_dir, config.dataset), download=True)` (src/train.py:134-147, src/data_loaders.py:50,82).
torchvision is not part of this stack and nothing is ever downloaded here: `load_cifar` parses the
published files itself, in either form, whichever is present under `root`:

  python form (what torchvision's download leaves behind)
    CIFAR10   root/cifar-10-batches-py/data_batch_1 .. data_batch_5, test_batch   keys data, labels
    CIFAR100  root/cifar-100-python/train, test                                   keys data, fine_labels
  binary form
    CIFAR10   root/cifar-10-batches-bin/data_batch_1.bin .. 5.bin, test_batch.bin records of 1 + 3072 bytes
    CIFAR100  root/cifar-100-binary/train.bin, test.bin          records of 2 + 3072 bytes (coarse, fine label)

Both store an image as 3072 bytes, planar: 1024 red, 1024 green, 1024 blue, each 32 rows of 32. The
images are returned exactly so, uint8 [n, 3, 32, 32]: the device transform reads the planar layout
directly (vit_preprocess_u8_gather, VIT_IMAGES_CHW), so the host never transposes the set.

The python form is a pickle, and a pickle can run anything. The files are therefore read with an
Unpickler that resolves only the four globals a numpy array needs and refuses every other one
before it is imported; plain `pickle.load` is never called on a dataset file.
"""
from __future__ import annotations

import io
import os
import pickle

import numpy as np

SUPPORTED = ("CIFAR10", "CIFAR100")
RECORD = 3 * 32 * 32

# name -> (python dir, train files, test files, label key, meta file, meta key,
#          binary dir, train files, test files, label bytes per record, meta file)
_SPEC = {
    "CIFAR10": dict(py_dir="cifar-10-batches-py", py_train=[f"data_batch_{i}" for i in range(1, 6)],
                    py_test=["test_batch"], label_key="labels", py_meta="batches.meta", meta_key="label_names",
                    bin_dir="cifar-10-batches-bin", bin_train=[f"data_batch_{i}.bin" for i in range(1, 6)],
                    bin_test=["test_batch.bin"], label_bytes=1, bin_meta="batches.meta.txt", classes=10),
    "CIFAR100": dict(py_dir="cifar-100-python", py_train=["train"], py_test=["test"], label_key="fine_labels",
                     py_meta="meta", meta_key="fine_label_names",
                     bin_dir="cifar-100-binary", bin_train=["train.bin"], bin_test=["test.bin"], label_bytes=2,
                     bin_meta="fine_label_names.txt", classes=100),
}


class DatasetError(RuntimeError):
    pass


def _numpy_globals():
    """the only globals a pickled ndarray refers to. Files written by numpy 1 name the reconstructor
    numpy.core.multiarray._reconstruct, numpy 2 numpy._core.multiarray._reconstruct: both map to the function
    this numpy pickles its own arrays with, so neither module is imported by name (numpy.core is a deprecated
    alias on numpy 2)"""
    import _codecs
    rec = np.zeros(0, np.uint8).__reduce__()[0]
    return {
        ("numpy.core.multiarray", "_reconstruct"): rec,
        ("numpy._core.multiarray", "_reconstruct"): rec,
        ("numpy", "ndarray"): np.ndarray,
        ("numpy", "dtype"): np.dtype,
        ("_codecs", "encode"): _codecs.encode,
    }


class _ArrayUnpickler(pickle.Unpickler):
    """Unpickler for the CIFAR python files: numpy arrays, lists, dicts, strings, numbers - nothing else"""

    _allowed = None

    def find_class(self, module, name):
        if _ArrayUnpickler._allowed is None:
            _ArrayUnpickler._allowed = _numpy_globals()
        try:
            return _ArrayUnpickler._allowed[(module, name)]
        except KeyError:
            raise pickle.UnpicklingError(
                f"dataset file names the global {module}.{name}: only numpy arrays are allowed in a CIFAR file, "
                "refusing to load it") from None


def _unpickle(path):
    """the dict of one python-form file (written by Python 2: latin1 strings)"""
    with open(path, "rb") as f:
        try:
            obj = _ArrayUnpickler(io.BytesIO(f.read()), encoding="latin1").load()
        except pickle.UnpicklingError:
            raise
        except Exception as e:  # a truncated or foreign file
            raise DatasetError(f"{path}: not a CIFAR python-form file ({type(e).__name__}: {e})") from e
    if not isinstance(obj, dict):
        raise DatasetError(f"{path}: expected a dict, found {type(obj).__name__}")
    return obj


def _read_python(path, label_key):
    d = _unpickle(path)
    if "data" not in d or label_key not in d:
        raise DatasetError(f"{path}: keys 'data' and {label_key!r} expected, found {sorted(map(str, d))}")
    data = np.asarray(d["data"])
    if data.dtype != np.uint8 or data.ndim != 2 or data.shape[1] != RECORD:
        raise DatasetError(f"{path}: data must be uint8 [n, {RECORD}], found {data.dtype} {data.shape}")
    labels = np.asarray(d[label_key], dtype=np.int64).reshape(-1)
    if labels.shape[0] != data.shape[0]:
        raise DatasetError(f"{path}: {data.shape[0]} images but {labels.shape[0]} labels")
    return data, labels


def _read_binary(path, label_bytes):
    rec = label_bytes + RECORD
    size = os.path.getsize(path)
    if size == 0 or size % rec:
        raise DatasetError(f"{path}: {size} bytes is not a whole number of {rec}-byte records (truncated?)")
    raw = np.fromfile(path, dtype=np.uint8)
    if raw.size != size:
        raise DatasetError(f"{path}: read {raw.size} of {size} bytes")
    raw = raw.reshape(size // rec, rec)
    # the label is the last label byte: CIFAR-100 stores (coarse, fine)
    return raw[:, label_bytes:], raw[:, label_bytes - 1].astype(np.int64)


def _class_names(spec, base, form):
    """class names from the meta file, or None when it is absent"""
    if form == "python":
        path = os.path.join(base, spec["py_meta"])
        if not os.path.isfile(path):
            return None
        names = _unpickle(path).get(spec["meta_key"])
        return None if names is None else [n.decode("latin1") if isinstance(n, bytes) else str(n) for n in names]
    path = os.path.join(base, spec["bin_meta"])
    if not os.path.isfile(path):
        return None
    with open(path, "r", encoding="latin1") as f:
        return [line.strip() for line in f if line.strip()]


def load_cifar(root, name, train=True):
    """(images uint8 [n, 3, 32, 32] planar as stored, labels int64 [n], class names or None) of the
    train or test split of CIFAR10 / CIFAR100 under `root` (= os.path.join(data_dir, dataset)).
    Files are concatenated in their published order (data_batch_1 .. 5). Nothing is downloaded: a missing
    directory raises DatasetError naming the paths that were tried."""
    if name not in _SPEC:
        raise DatasetError(f"dataset {name!r} is not supported: this loader reads {' and '.join(SUPPORTED)} "
                           "(ImageNet / TinyImageNet need JPEG decoding, which is outside this path)")
    spec = _SPEC[name]
    py_base, bin_base = os.path.join(root, spec["py_dir"]), os.path.join(root, spec["bin_dir"])
    if os.path.isdir(py_base):
        form, base, files = "python", py_base, spec["py_train" if train else "py_test"]
    elif os.path.isdir(bin_base):
        form, base, files = "binary", bin_base, spec["bin_train" if train else "bin_test"]
    else:
        raise DatasetError(f"{name} not found: looked for {py_base} and {bin_base} (nothing is downloaded here; "
                           "unpack the published archive under --data-dir/<dataset>/)")
    parts = []
    for fn in files:
        path = os.path.join(base, fn)
        if not os.path.isfile(path):
            raise DatasetError(f"{name}: {path} is missing")
        parts.append(_read_python(path, spec["label_key"]) if form == "python"
                     else _read_binary(path, spec["label_bytes"]))
    counts = {len(d) for d, _ in parts}
    if len(counts) != 1:
        raise DatasetError(f"{name}: the files under {base} hold different record counts "
                           f"{[len(d) for d, _ in parts]}")
    images = np.ascontiguousarray(np.concatenate([d for d, _ in parts])).reshape(-1, 3, 32, 32)
    labels = np.concatenate([l for _, l in parts])
    if labels.size and (labels.min() < 0 or labels.max() >= spec["classes"]):
        raise DatasetError(f"{name}: labels span [{labels.min()}, {labels.max()}], expected [0, {spec['classes']})")
    return images, labels, _class_names(spec, base, form)


# ---------------------------------------------------------------------------------------------------------
# Image folders: ImageNet (src/data_loaders.py:96-124, res-vit/data_loaders.py:188-216: torchvision's
# ImageFolder over <data-dir>/ImageNet/{train,val}) and TinyImageNet (res-vit/data_loaders.py:96-185: its own
# walk over <class>/images/). Only the file lists are made here; decoding is decode_rgb, one file at a time, and
# the resize happens on the device (vit_preprocess_u8_ragged), so images keep the sizes they have on disk.

IMG_EXTENSIONS = (".jpg", ".jpeg", ".png", ".ppm", ".bmp", ".pgm", ".tif", ".tiff", ".webp")
TINY_EXTENSIONS = (".png", ".jpg", ".jpeg")


def _class_dirs(root, what):
    if not os.path.isdir(root):
        raise DatasetError(f"{what} not found: looked for the directory {root} (nothing is downloaded or created "
                           "here)")
    with os.scandir(root) as it:
        return sorted(e.name for e in it if e.is_dir())


def find_image_folder(root):
    """(paths [n], labels int64 [n], classes) of the images under `root`, one sub-directory per class, under
    the rules of torchvision's `ImageFolder` (`datasets.folder.find_classes` / `make_dataset`). torchvision is
    not importable here, so the rules are restated, not called: the classes are the sorted names of the
    directories directly under root, class i gets label i; per class, in class order, the directory is walked
    with `sorted(os.walk(dir, followlinks=True))` and within each directory the sorted file names are taken;
    a file is kept when its lower-cased extension is one of IMG_EXTENSIONS. A class directory without any image
    is an error, as it is in torchvision, and so is a root without class directories."""
    classes = _class_dirs(root, "image folder")
    if not classes:
        raise DatasetError(f"{root} holds no class directories (expected {root}/<class>/<image files>)")
    paths, labels, empty = [], [], []
    for idx, cls in enumerate(classes):
        before = len(paths)
        for d, _, names in sorted(os.walk(os.path.join(root, cls), followlinks=True)):
            for fn in sorted(names):
                if fn.lower().endswith(IMG_EXTENSIONS):
                    paths.append(os.path.join(d, fn))
                    labels.append(idx)
        if len(paths) == before:
            empty.append(cls)
    if empty:
        raise DatasetError(f"{root}: found no image file for the class{'es' if len(empty) > 1 else ''} "
                           f"{', '.join(empty[:5])}{' ...' if len(empty) > 5 else ''} (extensions "
                           f"{', '.join(IMG_EXTENSIONS)})")
    return paths, np.asarray(labels, np.int64), classes


def find_tiny_imagenet(root, split):
    """(paths, labels int64, classes) of the `split` ('train', 'val' or 'test') of TinyImageNet under `root`,
    as res-vit/data_loaders.py:124-152 lists it: the classes are `sorted(os.listdir(root/split))`, class i gets
    label i, and the samples of a class are the .png / .jpg / .jpeg files of `<class>/images/`. The reference
    takes them in `os.listdir` order, which depends on the file system and cannot be reproduced by anyone; here
    they are taken in sorted order, so the list is the same on every machine (the evaluation result does not
    depend on the order, the shuffled training order does).
    The published download stores its validation split differently: `val/images/*.JPEG` plus
    `val/val_annotations.txt` (file name, class id, box). On that form the reference's walk finds the single
    'class' images with no samples; here it is read: the label of a file is the position of its class id among
    the sorted class ids of `root/train`, the files are taken in sorted order."""
    base = os.path.join(root, split)
    annotations = os.path.join(base, "val_annotations.txt")
    if os.path.isfile(annotations) and os.path.isdir(os.path.join(base, "images")):
        classes = _class_dirs(os.path.join(root, "train"), "TinyImageNet train split (its class ids label the "
                              "annotated validation files)")
        index = {c: i for i, c in enumerate(classes)}
        wnid = {}
        with open(annotations, "r", encoding="utf-8") as f:
            for line in f:
                parts = line.split()
                if len(parts) >= 2:
                    wnid[parts[0]] = parts[1]
        paths, labels = [], []
        for fn in sorted(os.listdir(os.path.join(base, "images"))):
            if not fn.lower().endswith(TINY_EXTENSIONS):
                continue
            if fn not in wnid:
                raise DatasetError(f"{annotations} has no line for {fn}")
            if wnid[fn] not in index:
                raise DatasetError(f"{annotations}: {fn} is labelled {wnid[fn]}, which is no directory of "
                                   f"{os.path.join(root, 'train')}")
            paths.append(os.path.join(base, "images", fn))
            labels.append(index[wnid[fn]])
    else:
        if not os.path.isdir(base):
            raise DatasetError(f"TinyImageNet {split} split not found: looked for the directory {base} (nothing "
                               "is downloaded or created here)")
        classes = sorted(os.listdir(base))
        paths, labels = [], []
        for idx, cls in enumerate(classes):
            d = os.path.join(base, cls, "images")
            if os.path.isdir(d):
                for fn in sorted(os.listdir(d)):
                    if fn.lower().endswith(TINY_EXTENSIONS):
                        paths.append(os.path.join(d, fn))
                        labels.append(idx)
    if not paths:
        raise DatasetError(f"{base} holds no image: expected <class>/images/*.JPEG, or images/ with "
                           "val_annotations.txt")
    return paths, np.asarray(labels, np.int64), classes


def decode_rgb(path):
    """The reference's loader, `PIL.Image.open(path).convert('RGB')` (torchvision's `pil_loader`,
    res-vit/data_loaders.py:169), as uint8 [H, W, 3]: grayscale, palette, RGBA and CMYK files become RGB by
    Pillow's own rules. Pillow is the decoder and is imported here, not with the module, so everything else in
    this file works without it."""
    try:
        from PIL import Image
    except ImportError as e:
        raise DatasetError(f"decoding image files needs Pillow (PIL), which is not importable here: {e}") from e
    try:
        with open(path, "rb") as f:
            with Image.open(f) as im:
                a = np.asarray(im.convert("RGB"), dtype=np.uint8)
    except Exception as e:  # a truncated or foreign file, or one that is not there
        raise DatasetError(f"{path}: cannot be decoded as an image ({type(e).__name__}: {e})") from e
    if a.ndim != 3 or a.shape[2] != 3 or a.shape[0] == 0 or a.shape[1] == 0:
        raise DatasetError(f"{path}: decoded to shape {a.shape}, expected [H, W, 3]")
    return np.ascontiguousarray(a)
