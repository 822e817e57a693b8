"""The launch-plan choices that are still open: one frozen record per model.

``Reconstructor.options`` holds it (a plain attribute, like ``precision``) and it is part of the engine stamp: assigning
``net.options = dataclasses.replace(net.options, fuse_inc=False)`` rebuilds the engines and drops captured graphs.  Every leg
behind a field is a real fallback the engines take for other shapes or formats as well; the defaults are what the A/B records
cited below chose.  ``SFH_OPTIONS`` is read once per model, by ``Reconstructor.__init__``.
"""
import os
from dataclasses import dataclass, fields

_LEVELS = frozenset({1, 2, 3, 4})


@dataclass(frozen=True)
class Options:
    # the UNet's first DoubleConv as one launch (csrc/conv_inc_fused.hip), f16x3 only: profiles/ab_inc_fused.txt
    fuse_inc: bool = True
    # ConvTranspose2d folded into the Up block's first conv, split formats only ("Fused Up block")
    fuse_up: bool = True
    # OutConv in the epilogue of the last 3x3 conv, split formats only: +0.6 % (outconv_kernel)
    fuse_head: bool = True
    # Up levels whose fused first conv runs as ONE kernel (csrc/conv_upfused.hip), f16x3 only: profiles/r05_ab_up_single.txt
    up_single: frozenset = frozenset({3, 4})
    # split-K for the ResNet-STN launches that fill at most a quarter of the chip: profiles/r03_resnet_table_*.txt
    splitk: bool = True
    # training: the one-pass forms (BatchNorm + ReLU + pool, transposed-conv s2d + bias sums, first-layer BatchNorm backward
    # in the backward-filter kernel, backward sums from the transposed conv / the OutConv): profiles/r05_ab_train_fusions.txt
    train_one_pass: bool = True

    def __post_init__(self):
        object.__setattr__(self, "up_single", frozenset(self.up_single))
        if not self.up_single <= _LEVELS:
            raise ValueError(f"up_single={sorted(self.up_single)}: Up levels are 1..4")

    @classmethod
    def parse(cls, text):
        """'name=value:name=value' -> Options; booleans are 0 / 1, up_single a digit string ('' = no level)"""
        names = [f.name for f in fields(cls)]
        kw = {}
        for item in text.split(":") if text else ():
            name, eq, val = item.partition("=")
            if not eq or name not in names:
                raise ValueError(f"SFH_OPTIONS: {item!r} is not name=value with a name of {names}")
            if name == "up_single":
                if not all(c in "1234" for c in val):
                    raise ValueError(f"SFH_OPTIONS: up_single={val!r}: digits of the Up levels 1..4 expected ({names})")
                kw[name] = frozenset(int(c) for c in val)
            elif val in ("0", "1"):
                kw[name] = val == "1"
            else:
                raise ValueError(f"SFH_OPTIONS: {name}={val!r}: 0 or 1 expected ({names})")
        return cls(**kw)

    @classmethod
    def from_env(cls):
        return cls.parse(os.environ.get("SFH_OPTIONS", ""))
