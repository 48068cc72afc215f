"""The pins of test_isa_guard.py::test_wfold_pass_is_what_the_design_says for EVERY instantiation of wfold_pass_kernel, the SLOTS
ones included (CPU-only: hipcc cross-compiles).  That test takes the first symbol that matches a (field, KF, KS, NT) fragment, which
is the kernel without slots; the kernel that runs by default on large tables is the one with them: two waves per SIMD, at most
256 VGPRs, nothing in scratch and no spills (the held-back outputs are 16 / 8 statically indexed VGPRs), 128-160 KiB of LDS, the
nontemporal hint on the NT instances' table loads and on no access of the others, and the eight loads of a sub-step in one batch."""
import os
import re
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "thaler-study_amd", "csrc")
FIELDS = ("14GoldilocksMontE", "11MontGenericE")
SHAPES = ((4, 5), (5, 3), (5, 4), (5, 5))


@pytest.fixture(scope="module")
def isa():
    subprocess.check_call(["make", "-C", CSRC, "isa"], stdout=subprocess.DEVNULL)
    text = open(os.path.join(CSRC, "build", "sumcheck_hip.s")).read()
    usage = open(os.path.join(CSRC, "build", "resource_usage.txt")).read()
    return text, usage


def symbol(fld, kf, ks, nt, slots):
    return "wfold_pass_kernelINS_%sLi%dELi%dELb%dELb%dEEEv" % (fld, kf, ks, nt, slots)


def usage_of(usage, frag):
    blocks = [b for b in usage.split("remark: Function Name: ")[1:] if frag in b.split(" ")[0]]
    assert len(blocks) == 1, (frag, len(blocks))
    return {key: int(re.search(re.escape(key) + r": (\d+)", blocks[0]).group(1))
            for key in ("VGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "LDS Size [bytes/block]", "VGPRs Spill", "SGPRs Spill")}


def body_of(text, frag):
    m = re.search(r"^(_ZN2sc\S*%s\S*):[^\n]*\n(.*?)\n\.Lfunc_end" % re.escape(frag), text, flags=re.S | re.M)
    assert m, frag
    return m.group(2)


@pytest.mark.parametrize("slots", [0, 1])
def test_every_wfold_instantiation_keeps_the_pins(isa, slots):
    text, usage = isa
    for fld in FIELDS:
        for kf, ks in SHAPES:
            for nt in (0, 1):
                frag = symbol(fld, kf, ks, nt, slots)
                u = usage_of(usage, frag)
                assert u["ScratchSize [bytes/lane]"] == 0 and u["VGPRs Spill"] == 0, (frag, u)
                assert u["SGPRs Spill"] <= (0 if fld == FIELDS[0] else 4), (frag, u)
                assert u["Occupancy [waves/SIMD]"] == 2 and u["VGPRs"] <= 256, (frag, u)
                assert 128 * 1024 <= u["LDS Size [bytes/block]"] <= 160 * 1024, (frag, u)
                body = body_of(text, frag)
                assert "scratch_" not in body, frag
                loads = [l for l in re.findall(r"global_load_dwordx4[^\n]*", body) if "sc0 sc1" not in l]   # (not the exchange's poll)
                stores = re.findall(r"global_store_dwordx4[^\n]*", body)
                if nt:
                    assert len(loads) >= 64 and all(" nt" in l for l in loads), frag
                else:
                    assert not any(" nt" in l for l in loads + stores), frag
                best = run = 0
                for l in (x.strip() for x in body.split("\n")):
                    if l.startswith("global_load_dwordx4"):
                        run += 1
                        best = max(best, run)
                    elif l.startswith(("ds_", "s_waitcnt", "s_barrier", "v_mad", "v_mul")):
                        run = 0
                assert best >= 8, (frag, best)


def test_the_slots_look_at_the_clock_and_hold_their_outputs_in_registers(isa):
    """a SLOTS kernel reads the wall clock once when it starts and once at each of a tile's four boundaries (the kernel without
    them only in the spin limit of its in-kernel exchange), and has the stores of every way out of the registers: the four
    boundaries, the deadline and the loop's end, four 16-byte stores each for KF = 4, besides the four direct ones (width 0)"""
    text, _ = isa
    for fld in FIELDS:
        with_slots = body_of(text, symbol(fld, 4, 5, 1, 1))
        without = body_of(text, symbol(fld, 4, 5, 1, 0))
        assert with_slots.count("s_memrealtime") >= without.count("s_memrealtime") + 5, fld
        assert with_slots.count("global_store_dwordx4") >= without.count("global_store_dwordx4") + 4 * 6, fld
