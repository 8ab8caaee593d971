"""The reference's YAML settings loader (utils/config_utils.py:4-50): ``load_config(path)`` reads a scene's file and lays it over the
file its ``inherit_from`` names, recursively.

``inherit_from`` is a relative path.  The reference resolves it against the working directory (its files say
``configs/mono/KITTI/base_config.yaml`` and expect to be run from the checkout's root).  Here it is looked for, in this order: as an
absolute path; under the directory of the inheriting file and each of its ancestors (so a ``configs/`` tree works wherever it lies and
whatever the working directory is); under the working directory.  A parent that is nowhere raises ``FileNotFoundError``, a chain that
comes back to a file it has already read raises ``ValueError`` (the reference would recurse until the interpreter stops it)."""
import os

import yaml


def _resolve(inherit_from, child):
    if os.path.isabs(inherit_from):
        if os.path.isfile(inherit_from):
            return inherit_from
        raise FileNotFoundError(f"{child}: inherit_from {inherit_from!r} does not exist")
    d = os.path.dirname(os.path.abspath(child))
    while True:
        cand = os.path.join(d, inherit_from)
        if os.path.isfile(cand):
            return cand
        up = os.path.dirname(d)
        if up == d:
            break
        d = up
    if os.path.isfile(inherit_from):
        return os.path.abspath(inherit_from)
    raise FileNotFoundError(f"{child}: inherit_from {inherit_from!r} found neither beside the file or above it nor under {os.getcwd()}")


def update_recursive(dict1, dict2):
    """``dict2`` laid over ``dict1`` in place: a dict value descends, anything else replaces (utils/config_utils.py:36-50)."""
    for k, v in dict2.items():
        if k not in dict1:
            dict1[k] = dict()
        if isinstance(v, dict):
            update_recursive(dict1[k], v)
        else:
            dict1[k] = v


def load_config(path, default_path=None, _seen=()):
    """The merged settings of ``path``: its ``inherit_from`` chain first (or ``default_path`` where a file names no parent), the file
    itself on top.  The ``inherit_from`` key stays in the result, as in the reference."""
    real = os.path.realpath(path)
    if real in _seen:
        raise ValueError("load_config: inherit_from cycle: " + " -> ".join(_seen + (real,)))
    with open(path, "r") as f:
        special = yaml.full_load(f) or {}
    inherit_from = special.get("inherit_from")
    if inherit_from is not None:
        cfg = load_config(_resolve(inherit_from, path), default_path, _seen + (real,))
    elif default_path is not None:
        with open(default_path, "r") as f:
            cfg = yaml.full_load(f) or {}
    else:
        cfg = dict()
    update_recursive(cfg, special)
    return cfg
