"""``engine.WS_HEADER`` against ``WsHeader`` of csrc/workspace.h as the C++ compiler lays it out."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ws_header_dtype_matches_the_struct(tmp_path):
    """A host-only program prints sizeof(WsHeader), kHistPartOff and offset / size of every field
    the dtype names; names, offsets, item sizes and the total size must agree, and the named fields
    must tile the struct (so it has no field the dtype leaves out)."""
    from structured_light_for_3d_model_replication_amd import build, engine as E
    names = list(E.WS_HEADER.names)
    lines = ["#include <stdio.h>", f'#include "{build.CSRC}/workspace.h"', "int main() {",
             '  printf("sizeof %zu\\n", sizeof(WsHeader));',
             '  printf("room %lld\\n", (long long)kHistPartOff);']
    for f in names:
        lines.append(f'  printf("{f} %zu %zu\\n", offsetof(WsHeader, {f}), sizeof(WsHeader::{f}));')
    lines.append("  return 0;\n}")
    src = tmp_path / "ws_header.cpp"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "ws_header"
    subprocess.run([build.HIPCC, "-x", "hip", "--cuda-host-only", "-std=c++17", "-o", str(exe), str(src)], check=True)
    got = {}
    for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines():
        key, *vals = line.split()
        got[key] = [int(v) for v in vals]
    assert got.pop("sizeof") == [E.WS_HEADER.itemsize]
    assert got.pop("room") == [E.WS_HEADER_BYTES] and E.WS_HEADER.itemsize <= E.WS_HEADER_BYTES
    assert list(got) == names
    end = 0
    for f in names:
        dt, off = E.WS_HEADER.fields[f][:2]
        assert got[f] == [off, dt.itemsize], f
        assert off == end, f"a gap or an unnamed field before {f}"
        end = off + dt.itemsize
    assert end == E.WS_HEADER.itemsize
    assert (E.WS_TOTALS_OFF, E.WS_ABOVE_OFF) == (got["totals"][0], got["above"][0])
