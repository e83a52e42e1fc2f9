"""Host side of weight_dtype 4 ("bf16_mfma"): the header's mode text, the engine's name table, infer.py's flag, and the bf16
fragment-major layout's index function (csrc/gemm_b16.h, exported as gvc_fb16_index) -- no GPU needed."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_documents_mode_4():
    header = open(os.path.join(ROOT, "include", "genvc_hip.h")).read()
    text = header[header.index("int32_t weight_dtype;"):header.index("} gvc_gpt_dims;")]
    assert re.search(r'\b4 \("bf16_mfma"\)', text)
    for word in ("v_mfma_f32_16x16x32_bf16", "csrc/gemm_b16.hip", "12 d^2 x 2 bytes per layer", "755 MB", "act_bf16_prefill"):
        assert word in text, word
    assert "gvc_gpt_bf16_gemm_launches" in header and "gvc_fb16_index" in header


def test_engine_name_table():
    from genvc_amd import engine
    assert engine.WEIGHT_DTYPES == {"fp32": 0, "bf16": 1, "bf16_kv": 2, "bf16_act": 3, "bf16_mfma": 4}


def test_infer_accepts_the_new_weights_name():
    run = lambda name: subprocess.run([sys.executable, os.path.join(ROOT, "infer.py"), "--weights", name, "--help"], capture_output=True,
                                      text=True, timeout=120, cwd=ROOT)
    ok, bad = run("bf16_mfma"), run("bf16_mfma_x")
    assert ok.returncode == 0 and "bf16_mfma" in ok.stdout, ok.stderr[-500:]
    assert bad.returncode != 0 and "invalid choice" in bad.stderr


def test_layout_index_is_a_bijection_and_follows_the_mfma_lane_map():
    """16x16x32 bf16 operand map: lane l holds row l & 15, k = 8 (l >> 4) + j in element j of its 16-byte fragment; a (16 rows x 32 k)
    block is the 64 fragments in lane order, 512 elements, blocks of one 16-row tile in k order"""
    from genvc_amd.build import build
    from genvc_amd import _lib
    build(verbose=False)
    idx = _lib.lib().gvc_fb16_index
    M, K = 32, 64
    seen = {int(idx(m, k, K)) for m in range(M) for k in range(K)}
    assert seen == set(range(M * K))
    for tile in range(M // 16):
        for kb in range(K // 32):
            base = (tile * (K // 32) + kb) * 512
            for lane in range(64):
                for j in range(8):
                    assert int(idx(tile * 16 + (lane & 15), kb * 32 + 8 * (lane >> 4) + j, K)) == base + lane * 8 + j
