"""The counter tools behind bench.py's roofline.valu_issue / traffic, run on the committed
round-3 counter passes (profiles/r03/r03j/pmc_b{8,16}, rocprofv3 CSVs of the shipped build)."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PMC = os.path.join(ROOT, "profiles", "r03", "r03j")


def _valu(tmp_path, block):
    out = tmp_path / "valu.json"
    ids = tmp_path / "ids.json"
    ids.write_text(json.dumps({"kernels": {}}))
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "valu.py"), os.path.join(PMC, f"pmc_b{block}"),
                    "--build", "test", "--ids", str(ids), "--out", str(out)], check=True, capture_output=True)
    return json.loads(out.read_text())["kernels"]


def test_valu_embed8_strip_and_list_pass(tmp_path):
    """embed<8>'s strip pass (embed_kernel<8, false>) gives the per-wave figures; its list pass
    (embed_kernel<8, true>) adds its issue cycles to the bound and its bytes to the traffic."""
    k = _valu(tmp_path, 8)
    e = k["embed_kernel<8>"]
    assert e["valu_instr_per_wave"] == 16615.4 and e["waves_per_frame"] == 4050.0
    assert e["list_pass"]["waves"] == 2048.0 and 0.0 < e["list_pass"]["issue_cycles_share"] < 0.05
    assert 75.0 < e["valu_issue_bound_us_per_frame"] < 90.0
    assert 49.9e6 < e["hbm_bytes_per_frame"] < 55e6
    x = k["extract_kernel<8>"]
    assert x["valu_instr_per_wave"] == 3608.2 and "list_pass" not in x


def test_valu_embed16(tmp_path):
    e = _valu(tmp_path, 16)["embed_kernel<16>"]
    assert e["valu_instr_per_wave"] == 39033.4 and "list_pass" not in e


def test_asm_diff_strips_and_counts():
    """tools/asm_diff.py compares code lines only: comments, directives, local labels and the
    per-unit __hip_cuid_* symbol do not count, a changed instruction counts on both sides."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import asm_diff
    finally:
        sys.path.pop(0)
    a = "\t.text\n; a comment\n_Z1kv:\n\ts_load_dword s0, s[4:5], 0x0\n.LBB0_1:\n\tv_add_f32 v0, v1, v2 ; kept\n\n__hip_cuid_1a2b:\n\ts_endpgm\n"
    same = "\t.amdgcn_target \"x\"\n_Z1kv:\n; another\n\ts_load_dword s0, s[4:5], 0x0\n.LBB0_7:\n\tv_add_f32 v0, v1, v2 ; kept\n__hip_cuid_ffff:\n\ts_endpgm\n\t.p2align 8\n"
    other = same.replace("v_add_f32 v0, v1, v2", "v_add_f32 v0, v2, v1") + "\ts_nop 0\n"
    assert asm_diff.strip_asm(a) == ["_Z1kv:", "s_load_dword s0, s[4:5], 0x0", "v_add_f32 v0, v1, v2 ; kept", "s_endpgm"]
    assert asm_diff.differing_lines(a, same) == 0
    assert asm_diff.differing_lines(a, other) == 3  # the instruction on both sides, and the added line
    assert asm_diff.differing_lines(a, "") == 4
