"""sfh_amd.options.Options: the one record of launch-plan choices, and the one environment variable behind it."""
import dataclasses
import glob
import os
import pickle
import re

import pytest

from sfh_amd.options import Options

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sports-field-homography_amd")


def test_defaults():
    assert dataclasses.asdict(Options()) == {
        "fuse_inc": True, "fuse_up": True, "fuse_head": True, "up_single": frozenset({3, 4}), "splitk": True,
        "train_one_pass": True}


def test_frozen_hashable_picklable():
    o = Options()
    with pytest.raises(dataclasses.FrozenInstanceError):
        o.fuse_inc = False
    p = dataclasses.replace(o, fuse_inc=False, up_single={4})
    assert p != o and hash(p) != hash(o) and hash(o) == hash(Options()) and len({o, Options(), p}) == 2
    assert isinstance(p.up_single, frozenset)
    assert pickle.loads(pickle.dumps(p)) == p


def test_from_env(monkeypatch):
    monkeypatch.delenv("SFH_OPTIONS", raising=False)
    assert Options.from_env() == Options()
    monkeypatch.setenv("SFH_OPTIONS", "fuse_inc=0:up_single=4")
    assert Options.from_env() == dataclasses.replace(Options(), fuse_inc=False, up_single=frozenset({4}))
    monkeypatch.setenv("SFH_OPTIONS", "up_single=")
    assert Options.from_env() == dataclasses.replace(Options(), up_single=frozenset())


@pytest.mark.parametrize("text", ["fuse_all=1", "fuse_inc", "fuse_inc=yes", "splitk=2", "up_single=5", "up_single=0",
                                  "fuse_inc=0:", "up_single=3,4"])
def test_from_env_rejects(monkeypatch, text):
    monkeypatch.setenv("SFH_OPTIONS", text)
    with pytest.raises(ValueError) as e:
        Options.from_env()
    for f in dataclasses.fields(Options):
        assert f.name in str(e.value)


def test_level_outside_the_unet_is_rejected():
    with pytest.raises(ValueError):
        Options(up_single={5})


def test_the_package_reads_the_environment_in_the_documented_places_only():
    found = {}
    for path in sorted(glob.glob(os.path.join(PKG, "*.py"))):
        with open(path) as f:
            n = len(re.findall(r"os\.environ|os\.getenv", f.read()))
        if n:
            found[os.path.basename(path)] = n
    assert found == {"_lib.py": 1, "sharding.py": 1, "build.py": 2, "reconstructor.py": 1, "training.py": 1, "options.py": 1}
