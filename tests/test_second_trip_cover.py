"""The ledger of capped loops (tests/second_trip.py) names kernels that exist in the source files it
names and cases that exist in tests/test_gpu_second_trip.py, or one of its written reasons.  No GPU
call: a renamed kernel or a removed case fails here."""
import os
import re

import second_trip as ST

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    "structured_light_for_3d_model_replication_amd", "csrc")


def test_every_named_kernel_exists_in_its_source_file():
    missing = []
    for src, kernel in ST.COVER:
        with open(os.path.join(CSRC, src)) as f:
            text = f.read()
        if not re.search(r"(?<![\w:])" + re.escape(kernel) + r"\s*\(", text):
            missing.append((src, kernel))
    assert not missing, missing


def test_every_named_case_exists():
    T = __import__(ST.CASES)
    cases = {v for v in ST.COVER.values() if v not in ST.REASONS}
    assert cases and all(v.startswith("test_") for v in cases)
    missing = sorted(c for c in cases if not callable(getattr(T, c, None)))
    assert not missing, missing
    assert T.pytestmark.name == "gpu"                     # the cases need the device; this file does not


def test_reasons_are_the_written_ones():
    assert {v for v in ST.COVER.values() if not v.startswith("test_")} == set(ST.REASONS)
    left_out = sorted(k for k, v in ST.COVER.items() if v == ST.REFERENCE_TOO_SLOW)
    assert left_out == [("cloud_orient.hip", "emst_far_kernel"), ("cloud_surface.hip", "candidates_kernel")]


def test_every_capped_stride_in_the_sources_is_in_the_ledger():
    """A loop that strides by the grid, or a one-workgroup loop over ``nb`` partials, sits in a
    kernel (or a shared body) the ledger names: a new one forces a decision."""
    stride = re.compile(r"for \(int(?:64_t)? (\w+) = blockIdx\.x; \1 < \w+; \1 \+= gridDim\.x\)"
                        r"|for \(int b = (?:t|threadIdx\.x); b < nb; b \+= 256\)"
                        r"|for \(int64_t base = 0; base < n_chunks; base \+= 1024\)")
    opener = re.compile(r"\bvoid (\w+)\(")            # the last function opened before the loop
    found = set()
    for src in sorted(os.listdir(CSRC)):
        if not src.endswith((".hip", ".h")):
            continue
        with open(os.path.join(CSRC, src)) as f:
            text = f.read()
        for m in stride.finditer(text):
            heads = [h for h in opener.finditer(text, 0, m.start())]
            assert heads, (src, m.group(0))
            found.add((src, heads[-1].group(1)))
    assert found and found <= set(ST.COVER), sorted(found - set(ST.COVER))
