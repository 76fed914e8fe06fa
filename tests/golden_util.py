"""Helpers to read the compact golden fixtures written by tests/golden/make_golden.py."""
import json
import os
from types import SimpleNamespace

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
STRIDE = 13
SHARD_BYTES = 900 << 10          # compressed bytes per fixture file: every file stays under 1 MiB
PART = "::part"                  # key suffix of the pieces of an array split along its first axis


def _shard_paths(name, directory=GOLDEN):
    """name.npz, name.1.npz, name.2.npz, ... that exist"""
    stem = os.path.join(directory, name[:-4])
    paths, i = [], 0
    while os.path.exists(stem + (".%d.npz" % i if i else ".npz")):
        paths.append(stem + (".%d.npz" % i if i else ".npz"))
        i += 1
    return paths


class Fixture:
    """A fixture stored as one or more .npz shards (name.npz, name.1.npz, ...), read like one NpzFile: `files`, `fx[key]`, `key in fx`.
    Arrays too large for one shard are stored in pieces along their first axis (key::part0, key::part1, ...) and joined here."""

    def __init__(self, paths):
        self._z = [np.load(p, allow_pickle=False) for p in paths]
        self._where, parts = {}, {}
        for z in self._z:
            for k in z.files:
                if PART in k:
                    base, i = k.rsplit(PART, 1)
                    parts.setdefault(base, []).append((int(i), z, k))
                else:
                    self._where[k] = z
        self._parts = {k: [z[n] for _, z, n in sorted(v, key=lambda e: e[0])] for k, v in parts.items()}
        self.files = list(self._where) + list(self._parts)

    def __getitem__(self, key):
        if key in self._parts:
            return np.concatenate(self._parts[key], 0)
        return self._where[key][key]

    def __contains__(self, key):
        return key in self._where or key in self._parts


def load(name):
    return Fixture(_shard_paths(name))


def _compressed_size(arrs):
    import io
    b = io.BytesIO()
    np.savez_compressed(b, **arrs)
    return b.tell()


def save(name, arrays, directory=GOLDEN):
    """Write `arrays` as the fixture `name` (read back by load()) in compressed shards of at most SHARD_BYTES."""
    items = []
    for k, v in arrays.items():
        v = np.asarray(v)
        size = _compressed_size({k: v})
        if size > SHARD_BYTES and v.ndim > 0 and v.shape[0] > 1:
            pieces = np.array_split(v, min(v.shape[0], -(-size // (SHARD_BYTES // 2))), 0)
            items += [(k + PART + str(i), p, _compressed_size({"p": p})) for i, p in enumerate(pieces)]
        else:
            items.append((k, v, size))
    shards, cur, used = [], {}, 0
    for k, v, size in items:
        if cur and used + size > SHARD_BYTES:
            shards.append(cur)
            cur, used = {}, 0
        cur[k] = v
        used += size
    shards.append(cur)
    for p in _shard_paths(name, directory):
        os.remove(p)
    stem = os.path.join(directory, name[:-4])
    for i, s in enumerate(shards):
        np.savez_compressed(stem + (".%d.npz" % i if i else ".npz"), **s)
    return len(shards)


def has(fx, key):
    return key in fx.files or (key + "::sub") in fx.files


def t(fx, key):
    return torch.from_numpy(np.asarray(fx[key]))


def check(fx, key, value, rtol=1e-5, atol=1e-6, what=""):
    """Compare tensor ``value`` with fixture entry ``key`` (full or compact form)."""
    value = value.detach().cpu()
    if key in fx.files:
        ref = t(fx, key)
        if ref.numel() == 0:
            assert value is None or value.numel() == 0 or float(value.abs().max()) == 0.0, key
            return
        torch.testing.assert_close(value.reshape(ref.shape).to(ref.dtype), ref, rtol=rtol, atol=atol, msg=lambda m: "%s %s: %s" % (what, key, m))
        return
    sub, stats = t(fx, key + "::sub"), fx[key + "::stats"]
    f = value.reshape(-1)
    assert f.numel() == int(stats[2]), (key, f.numel(), stats[2])
    torch.testing.assert_close(f[::STRIDE].to(sub.dtype), sub, rtol=rtol, atol=atol, msg=lambda m: "%s %s(sub): %s" % (what, key, m))
    asum = float(f.double().abs().sum())
    assert abs(asum - stats[1]) <= rtol * 10 * max(stats[1], 1.0) + atol * f.numel(), (key, asum, stats[1])
    assert abs(float(f.double().sum()) - stats[0]) <= rtol * 10 * max(stats[1], 1.0) + atol * f.numel(), (key, "sum")


def cfg_args(fx, tag, make_args, **extra):
    cfg = json.loads(str(fx[tag + ".cfg"]))
    return make_args("PEMS08", **cfg, **extra)
