"""CPU checks of csrc's layering, read from the sources as text: the units of
the extern "C" boundary (those that include lfm_api_internal.h) define no kernel and the kernel
units do not see lfm_api_internal.h; the large-N host units issue no copy or memset outside
`Copies`; and a factorising call's status word is decoded in one place."""

import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dis_project_amd", "csrc")
# the one listed exception: the farm's two helper kernels live beside its host code
EXCEPTION = {"lfm_farm.hip": {"stall_kernel", "farm_publish_kernel"}}
COPY_UNITS = ["lfm_api.hip", "lfm_post_api.hip"]


def _code(name):
    """The unit's text without comments and string literals."""
    with open(os.path.join(CSRC, name)) as f:
        text = f.read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r'"(?:\\.|[^"\\\n])*"', '""', text)
    return re.sub(r"//[^\n]*", "", text)


def _units():
    names = sorted(os.path.basename(p) for p in glob.glob(os.path.join(CSRC, "*.hip")))
    assert len(names) >= 16 and set(COPY_UNITS) <= set(names)
    return names


def _includes_api(name):
    with open(os.path.join(CSRC, name)) as f:
        return re.search(r'^#include "lfm_api_internal\.h"', f.read(), flags=re.M) is not None


def _kernels(name):
    code = re.sub(r"__launch_bounds__\s*\([^)]*\)", "", _code(name))
    return set(re.findall(r"__global__[^;{(]*?(\w+)\s*\(", code))


def test_units_of_the_c_boundary_define_no_kernel():
    api_units = [n for n in _units() if _includes_api(n)]
    assert set(COPY_UNITS) <= set(api_units)
    for name in api_units:
        assert _kernels(name) == EXCEPTION.get(name, set()), name


def test_kernel_units_do_not_see_the_c_boundarys_header():
    kernel_units = [n for n in _units() if "__global__" in _code(n)]
    assert "lfm_post.hip" in kernel_units and "lfm_sample.hip" in kernel_units
    for name in kernel_units:
        if name in EXCEPTION:
            assert _kernels(name) == EXCEPTION[name], name
        else:
            assert not _includes_api(name), name


def test_large_n_host_units_copy_through_copies_only():
    calls = ("hipMemcpyAsync(", "hipMemcpy2DAsync(", "hipMemsetAsync(")
    for name in COPY_UNITS:
        # none anywhere in their code, so no statement begins with one either (a discarded
        # result) and none is checked by hand: Copies (lfm_api_internal.h) is the one caller
        code = _code(name)
        assert "Copies " in code, name
        for c in calls:
            assert c not in code, (name, c)


def test_the_status_word_is_decoded_in_one_place():
    sites = []
    for name in _units() + ["lfm_api_internal.h", "lfm_internal.h"]:
        for m in re.finditer(r"\bstatus_code\(", _code(name)):
            line = _code(name)[: m.start()].count("\n") + 1
            sites.append((name, line))
    by_unit = {}
    for name, line in sites:
        by_unit.setdefault(name, []).append(line)
    # the declaration; the definition and result_tail's call; the restart pipeline's collect
    assert sorted(by_unit) == ["lfm_api.hip", "lfm_ctx.hip", "lfm_internal.h"], by_unit
    assert len(by_unit["lfm_internal.h"]) == 1
    assert len(by_unit["lfm_ctx.hip"]) == 2
    assert len(by_unit["lfm_api.hip"]) == 1
    code = _code("lfm_api.hip")
    collect = code.index("auto collect = ")
    call = code.index("status_code(")
    assert collect < call < code.index("auto drain = "), "status_code outside collect"
    ctx = _code("lfm_ctx.hip")
    tail = ctx.index("int result_tail(")
    assert ctx.index("status_code(", tail) < ctx.index("\n}\n", tail)
