"""The kernel source's layout: sunsky_kernels.hip is one translation unit made of the parts
under csrc/kernels/ (DESIGN.md "Kernel source map").  Compiles nothing.  CPU only."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import mk_probe  # noqa: E402

CSRC = os.path.join(ROOT, "mitsuba3-sunsky_amd", "csrc")
TOP = os.path.join(CSRC, "sunsky_kernels.hip")


def test_every_part_is_included_exactly_once():
    included = re.findall(r'^#include "kernels/([^"]+)"', open(TOP).read(), re.M)
    assert included, "sunsky_kernels.hip includes no part"
    assert sorted(included) == sorted(os.listdir(os.path.join(CSRC, "kernels")))   # none missing, none twice, none left out


@pytest.mark.parametrize("name", sorted(mk_probe.PROBES))
def test_probe_anchors_match_the_product_source(name):
    # make_source exits on an anchor that is missing or repeated in the expanded source
    text = mk_probe.make_source(name, TOP)
    assert '#include "kernels/' not in text
    assert text != mk_probe.product_source(TOP)


def test_no_tuning_hooks_in_the_kernel_source():
    for path in [TOP] + [os.path.join(CSRC, "kernels", f) for f in os.listdir(os.path.join(CSRC, "kernels"))]:
        assert "#ifndef SS_" not in open(path).read(), path
