"""What every generator of the gfx950 assembly kernels (gen_interp.py and the gen_*.py it drives) shares: the text buffer of one generator
run and that run's state, the experiment switches, the kernel record - entry label, descriptor and metadata entry of a kernel come from it
alone -, the instruction sequences that more than one kernel holds, and the registers that mean the same in all the interpreters."""
import dataclasses
import os
import re

# ---- experiment switches (FH_EXP, a comma-separated list; tools/build_variant.py): never set in a product build --------------------------
ROUTINES = ("sin", "cos", "tan", "asin", "acos", "atan", "exp", "ln")
SWITCHES = {
    "nointerp": "fh_columns: the set-up alone, no leaf is interpreted",
    "nodelta": "fh_columns: no delta handlers",
    "file64": "fh_columns: the default register map, a file of 64 registers behind 64 fixed ones",
    "nosqrt": "SQRT: v_sqrt_f32 alone (what the rounding of the root costs)",
    "twicesqrt": "SQRT: the sequence twice, same results",
    "nodiv": "DIV: a product in the division's place",
    "twicediv": "DIV: the sequence twice, same results",
    "nofastdiv": "DIV by an immediate: the general sequence",
    "compiledsincos": "fh_float_eval_*_t: SIN / COS by the compiled four-sample routines",
    "prune_nolive": "fh_prune1: no op counts as live but the OUTPUT ops",
}
SWITCHES.update({f"no{fn}": f"{fn.upper()}: a copy in the routine's place" for fn in ROUTINES})
SWITCHES.update({f"twice{fn}": f"{fn.upper()}: the compiled routine called twice, same results" for fn in ROUTINES})
VGPR_SWITCH = re.compile(r"vgpr(\d+)$")     # vgpr<N>: fh_columns declared with N registers (occupancy)


def parse_switches(text):
    """FH_EXP's text -> the set of its switches; a name that no generator knows ends the run"""
    names = frozenset(n for n in text.split(",") if n)
    for n in sorted(names):
        if n not in SWITCHES and not VGPR_SWITCH.match(n):
            raise SystemExit(f"FH_EXP: unknown switch '{n}' (known: {', '.join(sorted(SWITCHES))}, vgpr<N>)")
    return names


class Asm:
    """The text of one generator run and the run's state: the experiment switches, fh_columns' footprints per work item (FH_BLKL; capi.hip
    FH_COL_BLKL must agree), and the copies of the compiled routines embedded so far (gen_trans.embed), which fh_trans_probe reaches."""

    def __init__(self, exp=frozenset(), blkl=2):
        self.lines = []
        self.uid = 0
        self.exp, self.blkl = exp, blkl
        self.copies = []      # (prefix, v_base, routine names) of every gen_trans.embed()

    @classmethod
    def from_env(cls, env=os.environ):
        return cls(parse_switches(env.get("FH_EXP", "")), int(env.get("FH_BLKL", "2")))

    def __call__(self, s=""):
        for ln in s.strip("\n").split("\n"):
            self.lines.append(ln.rstrip())

    def label(self, stem):
        self.uid += 1
        return f".L{stem}_{self.uid}"

    def vgpr_switch(self):
        """N of the switch vgpr<N>, or None"""
        return next((int(m.group(1)) for m in map(VGPR_SWITCH.match, self.exp) if m), None)

    def text(self):
        return "\n".join(self.lines) + "\n"


def renamed(a, gen, uid_offset, renames, keep_uid=False):
    """the `_t` form of a kernel whose labels carry its name: gen(b) into a scratch buffer b of the same run (local labels numbered from
    a's + uid_offset), then the text with every (old, new) of `renames` replaced, in that order.  -> what gen returned"""
    b = Asm(a.exp, a.blkl)
    b.uid, b.copies = a.uid + uid_offset, a.copies
    r = gen(b)
    text = b.text()
    for old, new in renames:
        text = text.replace(old, new)
    a(text)
    if keep_uid:
        a.uid = max(a.uid, b.uid)
    return r


# ---- the kernel record -----------------------------------------------------------------------------------------------------------
PTR, U32 = (8, "global_buffer"), (4, "by_value")      # kernarg arguments


@dataclasses.dataclass
class Kernel:
    name: str
    args: list            # [(size, value kind)]: the kernarg segment is these, packed
    vgprs: int            # next free VGPR
    sgprs: int = 102      # next free SGPR
    wg_x: bool = True     # workgroup id x in s2 (y in s3)
    wg_y: bool = False
    lds: int = 0          # bytes, in the descriptor (the metadata entry says 0 for every kernel: the loader takes the descriptor's)

    @property
    def kernarg(self):
        return sum(size for size, _ in self.args)

    def begin(self, a):
        a(f"""
	.text
	.protected {self.name}
	.globl {self.name}
	.p2align 8
	.type {self.name},@function
{self.name}:""")

    def end(self, a):
        """s_endpgm, the kernel's size and its descriptor"""
        n = self.name
        a(f"""
	s_endpgm
.L{n}_end:
	.size {n}, .L{n}_end - {n}
	.rodata
	.p2align 6
	.amdhsa_kernel {n}
		.amdhsa_group_segment_fixed_size {self.lds}
		.amdhsa_private_segment_fixed_size 0
		.amdhsa_kernarg_size {self.kernarg}
		.amdhsa_user_sgpr_count 2
		.amdhsa_user_sgpr_kernarg_segment_ptr 1
		.amdhsa_system_sgpr_workgroup_id_x {int(self.wg_x)}
		.amdhsa_system_sgpr_workgroup_id_y {int(self.wg_y)}
		.amdhsa_system_sgpr_workgroup_id_z 0
		.amdhsa_system_vgpr_workitem_id 0
		.amdhsa_next_free_vgpr {self.vgprs}
		.amdhsa_next_free_sgpr {self.sgprs}
		.amdhsa_accum_offset {(self.vgprs + 3) // 4 * 4}
		.amdhsa_reserve_vcc 1
		.amdhsa_float_round_mode_32 0
		.amdhsa_float_round_mode_16_64 0
		.amdhsa_float_denorm_mode_32 3
		.amdhsa_float_denorm_mode_16_64 3
		.amdhsa_dx10_clamp 1
		.amdhsa_ieee_mode 1
	.end_amdhsa_kernel
	.text""")

    def metadata(self, a):
        a("  - .agpr_count:     0\n    .args:")
        offp = 0
        for size, kind in self.args:
            if kind == "global_buffer":
                a(f"      - .address_space:  global\n        .offset:         {offp}\n        .size:           {size}\n        .value_kind:     global_buffer")
            else:
                a(f"      - .offset:         {offp}\n        .size:           {size}\n        .value_kind:     by_value")
            offp += size
        a(f"""    .group_segment_fixed_size: 0
    .kernarg_segment_align: 8
    .kernarg_segment_size: {self.kernarg}
    .max_flat_workgroup_size: 64
    .name:           {self.name}
    .private_segment_fixed_size: 0
    .sgpr_count:     106
    .sgpr_spill_count: 0
    .symbol:         {self.name}.kd
    .uniform_work_group_size: 1
    .uses_dynamic_stack: false
    .vgpr_count:     {self.vgprs}
    .vgpr_spill_count: 0
    .wavefront_size: 64""")


def metadata(a, kernels):
    a("\t.amdgpu_metadata\n---\namdhsa.kernels:")
    for k in kernels:
        k.metadata(a)
    a("amdhsa.target:   amdgcn-amd-amdhsa--gfx950\namdhsa.version:\n  - 1\n  - 2\n...\n\t.end_amdgpu_metadata")


# ---- instruction sequences that more than one kernel holds -------------------------------------------------------------------------
def _halves(pair):
    lo, hi = re.fullmatch(r"s\[(\d+):(\d+)\]", pair).groups()
    return f"s{lo}", f"s{hi}"


def pcrel(a, pair, target, here, far=None, dst=None):
    """pair = the address of `target`, position-relative: `here` is the label that s_getpc_b64's result names.  The plain form adds an
    unsigned 32-bit distance, so the target lies behind `here`; far = a scratch pair: a signed distance, a target anywhere in the code
    object.  dst: the sum goes to that pair and `pair` keeps the address of `here` (for a second target: add_rel)."""
    a(f"\ts_getpc_b64 {pair}\n{here}:")
    add_rel(a, dst or pair, pair, target, here, far)


def add_rel(a, dst, pair, target, here, far=None):
    """dst = the address of `target`, from pair = the address of `here` (see pcrel)"""
    (lo, hi), (dlo, dhi) = _halves(pair), _halves(dst)
    if far:
        flo, fhi = _halves(far)
        return a(f"\ts_mov_b32 {flo}, {target} - {here}\n\ts_ashr_i32 {fhi}, {flo}, 31\n\ts_add_u32 {dlo}, {lo}, {flo}\n\ts_addc_u32 {dhi}, {hi}, {fhi}")
    a(f"\ts_add_u32 {dlo}, {lo}, {target} - {here}\n\ts_addc_u32 {dhi}, {hi}, 0")


def ieee_div(a, num, den, out, d, mask):
    """out = num / den, IEEE-correct: the div_scale / rcp / fma / div_fmas / div_fixup sequence (the compiler's own expansion);
    d: five scratch VGPRs, mask: an SGPR pair for the first v_div_scale_f32's; clobbers vcc; out may be num or den"""
    a(f"""
	v_div_scale_f32 {d[0]}, {mask}, {den}, {den}, {num}
	v_rcp_f32 {d[1]}, {d[0]}
	v_div_scale_f32 {d[2]}, vcc, {num}, {den}, {num}
	v_fma_f32 {d[3]}, -{d[0]}, {d[1]}, 1.0
	v_fmac_f32 {d[1]}, {d[3]}, {d[1]}
	v_mul_f32 {d[3]}, {d[2]}, {d[1]}
	v_fma_f32 {d[4]}, -{d[0]}, {d[3]}, {d[2]}
	v_fmac_f32 {d[3]}, {d[4]}, {d[1]}
	v_fma_f32 {d[0]}, -{d[0]}, {d[3]}, {d[2]}
	v_div_fmas_f32 {d[0]}, {d[0]}, {d[1]}, {d[3]}
	v_div_fixup_f32 {out}, {d[0]}, {den}, {num}""")


def ieee_sqrt(a, x, out, d, mask, sqrtc):
    """out = sqrtf(x), correctly rounded, for every x: v_sqrt_f32 (1 ulp), then one ulp either way by the sign of the exact residuals;
    arguments below 2^-96 (sqrtc holds that bound) scaled by 2^32 and the result by 2^-16, zeros / +inf passed through.
    d: six scratch VGPRs, mask: an SGPR pair; clobbers vcc"""
    a(f"""
	v_mul_f32 {d[0]}, 0x4f800000, {x}
	v_cmp_gt_f32 vcc, {sqrtc}, {x}
	s_nop 1
	v_cndmask_b32 {d[1]}, {x}, {d[0]}, vcc
	v_sqrt_f32 {d[0]}, {d[1]}
	s_nop 0
	v_add_u32 {d[2]}, -1, {d[0]}
	v_add_u32 {d[3]}, 1, {d[0]}
	v_fma_f32 {d[4]}, -{d[2]}, {d[0]}, {d[1]}
	v_fma_f32 {d[5]}, -{d[3]}, {d[0]}, {d[1]}
	v_cmp_ge_f32_e64 {mask}, 0, {d[4]}
	s_nop 1
	v_cndmask_b32_e64 {d[0]}, {d[0]}, {d[2]}, {mask}
	v_cmp_lt_f32_e64 {mask}, 0, {d[5]}
	s_nop 1
	v_cndmask_b32_e64 {d[0]}, {d[0]}, {d[3]}, {mask}
	v_mul_f32 {d[2]}, 0x37800000, {d[0]}
	v_cndmask_b32 {d[0]}, {d[0]}, {d[2]}, vcc
	v_mov_b32 {d[3]}, 0x260
	v_cmp_class_f32 vcc, {d[1]}, {d[3]}
	s_nop 1
	v_cndmask_b32 {out}, {d[0]}, {d[1]}, vcc""")


def round_half_away(a, x, out, d, mask):
    """out = roundf(x), half away from zero; d: two scratch VGPRs, mask: an SGPR pair; S_ABSM holds 0x7fffffff"""
    a(f"""
	v_trunc_f32 {d[0]}, {x}
	v_sub_f32 {d[1]}, {x}, {d[0]}
	v_cmp_ge_f32_e64 {mask}, |{d[1]}|, 0.5
	s_nop 1
	v_cndmask_b32_e64 {d[1]}, 0, 1.0, {mask}
	v_bfi_b32 {d[1]}, {S_ABSM}, {d[1]}, {x}
	v_add_f32 {out}, {d[0]}, {d[1]}""")


# ---- registers that mean the same in every kernel that uses them -------------------------------------------------------------------
# (what a kernel's launch leaves, the constants every interpreter keeps, and the dispatch's working set.  A name that two kernels give to
# different registers - S_LEN, S_K, S_ARENA, V_QNAN ... - stays with each of them; so does fh_prune1's whole working set.)
S_KERNARG = "s[0:1]"
S_WG = "s2"             # workgroup id x
S_STATE = "s[4:5]"      # FhRenderState*
S_SIGN = "s28"          # 0x80000000
S_ABSM = "s29"          # 0x7fffffff
S_HBASE = "s[42:43]"    # address of handler 0
S_TAPE = "s[44:45]"     # interpreter argument: first op
S_QA = 48               # s[48:55]  current batch of 4 ops
S_QB = 56               # s[56:63]  next batch
S_W0, S_W1 = "s64", "s65"   # the op's two words
S_CUR = "s[64:65]"
S_T0 = "s66"
S_OUT = "s67"
S_A = "s68"
S_T1 = "s69"
S_FETCH = "s[72:73]"
S_RET = "s[74:75]"
S_PC = "s[86:87]"
S_SAVE = "s[88:89]"
S_M = [f"s[{90 + 2 * j}:{91 + 2 * j}]" for j in range(4)]   # lane masks s[90:97]
V_LANE = "v0"

SRC0, SRC1, SRC2, DST = 1, 2, 4, 8      # s_set_gpr_idx_on: which operands are M0-relative
