"""Host code under AddressSanitizer + UBSan: liblfm's host-only logic
(dis_project_amd/csrc/lfm_host.cpp: x-layout detection, the factorisation's step plan, the
host mirror of the trailing update's unit enumeration, the side-CU helper's sizing and lead
clamp, schedule 3's launch plan (plan_s3, over 1344 shapes: the flag array's four regions and
every step's slots in them, workspace / X-buffer / matrix bounds, the lead units of each launch
counted by enumeration against the target its chain waits for, a_done's target, the helper's
share and its lead-free tail, the grids, the overlap mark; and three golden plans, the launches
the library issued before the plan existed, flops included), the small-problem path's layout
and plans (lfm_small_plan.h: small_map's regions disjoint, inside the map and aligned over every
(n, G, T) and mode, the fit map = the gradient map + three regions; plan_small_mll bounding
each member's map within the LDS limit over pairs of shapes; small_post_cols maximal;
plan_small_post's buffer regions, its passes covering every test column once as
small_post_kernel enumerates them, the covariance kernel's tile search, the rejections in
order; plan_small_pack's offsets; golden values from the library before the plans existed),
the device tenancy lock: mutual
exclusion, shared admission, cross-process waits and the turnstile) and the C++ oracle (oracle/lfm_cpu.cpp), built by tests/native/Makefile and run by
tests/native/host_check.cpp. CPU only."""

import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++ with libasan")
def test_host_code_under_asan_and_ubsan():
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tests", "native"), "asan"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "host_check: all passed" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
