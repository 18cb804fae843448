"""scripts/isa_diff.py: the splitter and the normaliser, on two small synthetic listings (no compiler, no GPU)."""
from scripts import isa_diff


def _kernel(sym, index, body):
    """One function as the compiler lists it: section and type directives, the label, the instructions, the kernel descriptor inside
    the function's range, the end label."""
    return f"""\t.section\t.text.{sym},"axG",@progbits,{sym},comdat
\t.globl\t{sym} ; -- Begin function {sym}
\t.p2align\t8
\t.type\t{sym},@function
{sym}: ; @{sym}
; %bb.0:
{body}\t.section\t.rodata,"a",@progbits
\t.p2align\t6, 0x0
\t.amdhsa_kernel {sym}
\t\t.amdhsa_group_segment_fixed_size 64
\t\t.amdhsa_kernarg_size {128 + 8 * index}
\t.end_amdhsa_kernel
\t.section\t.text.{sym},"axG",@progbits,{sym},comdat
.Lfunc_end{index}:
\t.size\t{sym}, .Lfunc_end{index}-{sym}
                                        ; -- End function
\t.set {sym}.num_vgpr, 12
; Kernel info:
; codeLenInByte = 24
"""


def _meta(sym, vgpr):
    return f"""  - .agpr_count:     0
    .args:
      - .name:           a
        .offset:         0
        .size:           128
    .group_segment_fixed_size: 64
    .name:           {sym}
    .private_segment_fixed_size: 0
    .sgpr_count:     20
    .symbol:         {sym}.kd
    .vgpr_count:     {vgpr}
"""


def _listing(order, bodies, cuid, note):
    text = '\t.amdgcn_target "amdgcn-amd-amdhsa--gfx950"\n'
    for i, sym in enumerate(order):
        text += _kernel(sym, i, bodies[sym](i, note))
    text += f"\t.type\t__hip_cuid_{cuid},@object ; @__hip_cuid_{cuid}\n__hip_cuid_{cuid}:\n\t.byte\t0\n"
    text += "\t.amdgpu_metadata\n---\namdhsa.kernels:\n" + "".join(_meta(sym, 12) for sym in order)
    return text + "amdhsa.target:   amdgcn-amd-amdhsa--gfx950\n...\n\t.end_amdgpu_metadata\n"


BODIES = {
    "_Z5alphav": lambda i, note: f"""\ts_load_dwordx2 s[0:1], s[0:1], 0x0 ; {note}
\t.loc\t1 {10 + i} 3
\tv_mov_b32_e32 v1, 0
\ts_cbranch_scc0 .LBB{i}_2
; %bb.1: {note}
\tv_add_u32_e32 v1, 1, v1
.LBB{i}_2:
\ts_endpgm
""",
    "_Z4betav": lambda i, note: f"""\tv_lshlrev_b32_e32   v0, 2, v0   ; {note}
\t;;#ASMSTART
\t1:
\tv_fmac_f32 v2, v0, v1
\ts_cbranch_scc1 1b
\t;;#ASMEND
\ts_endpgm
""",
}


def test_same_kernels_under_other_comments_cuid_and_order_are_identical():
    base = _listing(["_Z5alphav", "_Z4betav"], BODIES, "4e6ad1bbb72490bd", "base")
    new = _listing(["_Z4betav", "_Z5alphav"], BODIES, "da3ea229d1e0f6a3", "another comment")
    rows, bad = isa_diff.compare(base, new)
    assert bad == 0
    assert [(r[0], r[1]) for r in rows] == [("_Z4betav", "identical"), ("_Z5alphav", "identical")]
    for _, _, b, n in rows:                      # the metadata figures of both sides
        assert b == n == {"vgpr_count": "12", "sgpr_count": "20", "private_segment_fixed_size": "0", "group_segment_fixed_size": "64"}
    # the listing's instructions survive the normaliser, its comments and directives do not
    body = isa_diff.split_kernels(base)["_Z5alphav"]["body"]
    assert body == ["s_load_dwordx2 s[0:1], s[0:1], 0x0", "v_mov_b32_e32 v1, 0", "s_cbranch_scc0 .LBB_2", "v_add_u32_e32 v1, 1, v1", ".LBB_2:", "s_endpgm"]


def test_one_changed_instruction_is_reported_for_its_kernel_alone():
    base = _listing(["_Z5alphav", "_Z4betav"], BODIES, "4e6ad1bbb72490bd", "base")
    changed = dict(BODIES)
    changed["_Z4betav"] = lambda i, note: BODIES["_Z4betav"](i, note).replace("v_fmac_f32 v2, v0, v1", "v_fma_f32 v2, v1, v0, v2")
    new = _listing(["_Z5alphav", "_Z4betav"], changed, "da3ea229d1e0f6a3", "new")
    rows, bad = isa_diff.compare(base, new)
    assert bad == 1
    assert {r[0]: r[1] for r in rows} == {"_Z5alphav": "identical", "_Z4betav": "differs"}
    assert "v_fma_f32 v2, v1, v0, v2" in isa_diff.kernel_diff(base, new, "_Z4betav")


def test_a_kernel_on_one_side_only_is_reported_by_name():
    base = _listing(["_Z5alphav", "_Z4betav"], BODIES, "4e6ad1bbb72490bd", "base")
    new = _listing(["_Z5alphav"], BODIES, "4e6ad1bbb72490bd", "base")
    rows, bad = isa_diff.compare(base, new)
    assert bad == 1
    assert {r[0]: r[1] for r in rows} == {"_Z5alphav": "identical", "_Z4betav": "only in base"}
    rows, bad = isa_diff.compare(new, base)
    assert bad == 1 and ("_Z4betav", "only in working tree") in [(r[0], r[1]) for r in rows]


# the same arithmetic as the compiler lists it after a refactor that changes no result: operands of commutative instructions swapped,
# registers renumbered, two independent instructions in the other order
_GAMMA = """\tv_mul_f32_e32 v3, v1, v2
\tv_add_f32_e32 v4, v3, v0
\tv_mul_f32_e32 v5, v4, v4
\ts_cbranch_scc0 .LBB{i}_2
\tv_add_f32_e32 v5, v5, v3
.LBB{i}_2:
\ts_endpgm
"""
_GAMMA_REORDERED = """\tv_mul_f32_e32 v7, v2, v1
\tv_add_f32_e32 v6, v0, v7
\tv_mul_f32_e32 v5, v6, v6
\ts_cbranch_scc0 .LBB{i}_2
\tv_add_f32_e32 v5, v7, v5
.LBB{i}_2:
\ts_endpgm
"""


def _gamma_pair(new_body, new_vgpr=12):
    base = _listing(["_Z5alphav", "_Z5gammav"], dict(BODIES, _Z5gammav=lambda i, note: _GAMMA.format(i=i)), "4e6ad1bbb72490bd", "base")
    new = _listing(["_Z5alphav", "_Z5gammav"], dict(BODIES, _Z5gammav=lambda i, note: new_body.format(i=i)), "da3ea229d1e0f6a3", "new")
    return base, new.replace(_meta("_Z5gammav", 12), _meta("_Z5gammav", new_vgpr))


def test_swapped_operands_and_renamed_registers_are_reordered():
    rows, bad = isa_diff.compare(*_gamma_pair(_GAMMA_REORDERED))
    assert bad == 0
    assert {r[0]: r[1] for r in rows} == {"_Z5alphav": "identical", "_Z5gammav": "reordered"}


def test_reordered_plus_one_changed_mnemonic_or_one_changed_figure_differs():
    # as many instructions, one of them another one
    rows, bad = isa_diff.compare(*_gamma_pair(_GAMMA_REORDERED.replace("v_add_f32_e32 v5, v7, v5", "v_sub_f32_e32 v5, v7, v5")))
    assert bad == 1
    assert {r[0]: r[1] for r in rows} == {"_Z5alphav": "identical", "_Z5gammav": "differs"}
    # one instruction more
    rows, bad = isa_diff.compare(*_gamma_pair(_GAMMA_REORDERED.replace("\ts_endpgm", "\ts_nop 0\n\ts_endpgm")))
    assert bad == 1 and {r[0]: r[1] for r in rows}["_Z5gammav"] == "differs"
    # the same reordered text with one register more in the metadata
    rows, bad = isa_diff.compare(*_gamma_pair(_GAMMA_REORDERED, new_vgpr=13))
    assert bad == 1
    assert {r[0]: r[1] for r in rows} == {"_Z5alphav": "identical", "_Z5gammav": "differs"}
    g = [r for r in rows if r[0] == "_Z5gammav"][0]
    assert g[2]["vgpr_count"] == "12" and g[3]["vgpr_count"] == "13"


def test_mix_lists_the_mnemonics_whose_counts_differ_with_both_counts_and_totals():
    # one v_add_f32 becomes a v_sub_f32 and an s_nop is added: 6 -> 7 instructions (labels are none), three mnemonics move
    changed = _GAMMA_REORDERED.replace("v_add_f32_e32 v5, v7, v5", "v_sub_f32_e32 v5, v7, v5").replace("\ts_endpgm", "\ts_nop 0\n\ts_endpgm")
    base, new = _gamma_pair(changed)
    assert isa_diff.kernel_mix(base, new, "_Z5gammav") == ((6, 7), [("s_nop", 0, 1), ("v_add_f32_e32", 2, 1), ("v_sub_f32_e32", 0, 1)])
    # a kernel whose text is only reordered has equal totals and an empty table
    assert isa_diff.kernel_mix(*_gamma_pair(_GAMMA_REORDERED), "_Z5gammav") == ((6, 6), [])
