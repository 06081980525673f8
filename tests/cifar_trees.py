"""Tiny CIFAR-10 / CIFAR-100 trees in the two published on-disk forms, written from a seed (test helper for
tests/test_datasets_cpu.py and tests/test_dataset_gpu.py; no real CIFAR file is ever committed)."""
import os
import pickle

import numpy as np

PY_DIR = {"CIFAR10": "cifar-10-batches-py", "CIFAR100": "cifar-100-python"}
BIN_DIR = {"CIFAR10": "cifar-10-batches-bin", "CIFAR100": "cifar-100-binary"}


def make_split(name, n, seed):
    """(data uint8 [n, 3072], fine labels [n], coarse labels [n]); the coarse labels never equal the fine ones"""
    rng = np.random.default_rng(seed)
    data = rng.integers(0, 256, (n, 3072), dtype=np.uint8)
    classes = 10 if name == "CIFAR10" else 100
    fine = rng.integers(0, classes, n)
    coarse = (fine + 1 + rng.integers(0, 18, n)) % 20
    coarse = np.where(coarse == fine, (coarse + 1) % 20, coarse)
    return data, fine.astype(np.int64), coarse.astype(np.int64)


def write_tree(root, name, form, per_train_file=4, n_test=6, seed=0, meta=True):
    """Write `name` under `root` (= data_dir/name) in `form` ("python" | "binary"); returns
    {"train": (data, labels), "test": (data, labels)} in file order."""
    files = ([f"data_batch_{i}" for i in range(1, 6)] if name == "CIFAR10" else ["train"])
    n_train = per_train_file * len(files)
    tr = make_split(name, n_train, seed)
    te = make_split(name, n_test, seed + 1)
    base = os.path.join(root, (PY_DIR if form == "python" else BIN_DIR)[name])
    os.makedirs(base, exist_ok=True)

    def dump(fn, data, fine, coarse):
        if form == "python":
            d = {"data": data, "filenames": [f"img{i}.png" for i in range(len(data))]}
            if name == "CIFAR10":
                d["labels"] = [int(v) for v in fine]
            else:
                d["fine_labels"] = [int(v) for v in fine]
                d["coarse_labels"] = [int(v) for v in coarse]
            with open(os.path.join(base, fn), "wb") as f:
                pickle.dump(d, f, protocol=2)
        else:
            lab = fine[:, None] if name == "CIFAR10" else np.stack([coarse, fine], 1)
            rec = np.concatenate([lab.astype(np.uint8), data], 1)
            rec.tofile(os.path.join(base, fn + ".bin"))

    for i, fn in enumerate(files):
        s = slice(i * per_train_file, (i + 1) * per_train_file)
        dump(fn, tr[0][s], tr[1][s], tr[2][s])
    dump("test_batch" if name == "CIFAR10" else "test", *te)
    if meta:
        names = [f"class{i}" for i in range(10 if name == "CIFAR10" else 100)]
        if form == "python":
            key, fn = ("label_names", "batches.meta") if name == "CIFAR10" else ("fine_label_names", "meta")
            with open(os.path.join(base, fn), "wb") as f:
                pickle.dump({key: names}, f, protocol=2)
        else:
            fn = "batches.meta.txt" if name == "CIFAR10" else "fine_label_names.txt"
            with open(os.path.join(base, fn), "w") as f:
                f.write("\n".join(names) + "\n")
    return {"train": (tr[0], tr[1]), "test": (te[0], te[1])}
