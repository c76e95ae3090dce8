"""The one-shape library of tools/devbuild.sh compiles the same translation units as the product's Makefile: a unit that only
the Makefile names leaves the one-shape library with undefined symbols, which shows as a failed load, not as a failed build."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def makefile_units():
    text = open(os.path.join(ROOT, "gato_python_amd", "csrc", "Makefile")).read()
    var = {m.group(1): m.group(2) for m in re.finditer(r"^(HOST_SRCS|SRCS) := (.*)$", text, re.M)}
    words = var["SRCS"].replace("$(HOST_SRCS)", var["HOST_SRCS"]).split()
    assert all(w.endswith(".hip") for w in words), words
    return [w[:-4] for w in words]


def devbuild_units():
    text = open(os.path.join(ROOT, "tools", "devbuild.sh")).read()
    loops = re.findall(r"^for f in (.*); do$", text, re.M)
    assert len(loops) == 1, loops
    return loops[0].split()


def test_devbuild_compiles_every_unit_of_the_makefile():
    mk, dev = makefile_units(), devbuild_units()
    assert len(set(mk)) == len(mk) and len(set(dev)) == len(dev)
    assert set(mk) == set(dev), sorted(set(mk) ^ set(dev))
    csrc = os.path.join(ROOT, "gato_python_amd", "csrc")
    on_disk = {f[:-4] for f in os.listdir(csrc) if f.endswith(".hip")}
    assert set(mk) == on_disk, sorted(set(mk) ^ on_disk)
