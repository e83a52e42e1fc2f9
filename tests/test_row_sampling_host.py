"""CPU: the per-row sampling ABI (include/genvc_hip.h gvc_row_sampling, gvc_sample_rows, gvc_gpt_generate_rows) and the host-side
checks of the layers that use it (no GPU needed)."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "genvc_hip.h"
int main(void) {
    printf("%zu", sizeof(gvc_row_sampling));
#define F(n) printf(" %s=%zu", #n, offsetof(gvc_row_sampling, n));
    F(repetition_penalty) F(temperature) F(top_p) F(top_k) F(seed) F(rng_row) F(rng_step0)
    printf("\n");
    return 0;
}
"""


def test_row_sampling_ctypes_layout_equals_c_layout(tmp_path):
    """the ctypes struct the Python layers fill is the struct the library reads: sizeof / offsetof from the host compiler"""
    from genvc_amd import _lib
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no host C compiler")
    src = tmp_path / "probe.c"
    src.write_text(_PROBE)
    exe = tmp_path / "probe"
    subprocess.run([cc, "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    size = int(out[0])
    offs = dict(kv.split("=") for kv in out[1:])
    R = _lib.RowSampling
    assert size == C.sizeof(R) == 32
    assert {n: int(v) for n, v in offs.items()} == {n: getattr(R, n).offset for n, _ in R._fields_}
    assert offs["seed"] == "16"


def test_row_sampling_symbols_are_bound():
    from genvc_amd import _lib
    syms = _lib.exported_symbols()
    assert "gvc_sample_rows" in syms and "gvc_gpt_generate_rows" in syms
    assert C.POINTER(_lib.RowSampling) in _lib._SIGNATURES["gvc_gpt_generate_rows"][1]
    assert C.POINTER(_lib.RowSampling) in _lib._SIGNATURES["gvc_sample_rows"][1]


def test_row_sampling_array_from_settings():
    from genvc_amd.engine import row_sampling
    rows = [dict(repetition_penalty=2.0, temperature=0.85, top_p=0.85, top_k=15, seed=(1 << 63) + 5, rng_row=3, rng_step0=141),
            dict(repetition_penalty=1.0, temperature=1.0, top_p=1.0, top_k=1, seed=0, rng_row=0, rng_step0=0)]
    a = row_sampling(rows)
    assert len(a) == 2 and a[0].top_k == 15 and a[0].seed == (1 << 63) + 5 and a[0].rng_row == 3 and a[0].rng_step0 == 141
    assert abs(a[0].temperature - 0.85) < 1e-7 and a[1].top_k == 1


def test_stream_sessions_open_rejects_sampling_on_a_shared_scheduler():
    """StreamSessions(per_session_sampling=False) samples every session with the model config: open(sampling=...) must not be
    silently ignored (the check runs before any device work)"""
    from genvc_amd.streaming import StreamSessions
    ss = StreamSessions.__new__(StreamSessions)
    ss.per_session_sampling = False
    with pytest.raises(ValueError):
        ss.open(None, sampling=dict(top_k=15))
    with pytest.raises(ValueError):
        ss.open(None, seed=5)
