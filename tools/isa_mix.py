#!/usr/bin/env python3
"""Instruction mix of the hot loops of mcd::loglike_kernel, from the gfx950 ISA hipcc emits.

    python tools/isa_mix.py                 # compiles csrc/mcd_kernels.hip with -save-temps into /tmp, prints a table
    python tools/isa_mix.py --json OUT      # additionally writes the table as JSON (what bench.py's roofline block reads;
                                            # __graft_entry__.build() refreshes mcmc_dynamics_amd/csrc/isa_mix.json)

For every fast-path instantiation the hot loop nest is located (label .. backward branch) and its vector instructions are
counted per star-walker term.  The narrow-range mixture variants rescale their running product on every second 4-star
iteration (a block behind a scalar branch): their count is (2 x loop body + rescale block) / 8.  The prefetching BGFIXED
narrow-range instantiation runs 8-star iterations with the rescale inside the loop body; its bounded sub-variant (template
parameter BOUNDED, the last one of the mangled name) rescales every fourth 8-star iteration at C3's R = 32, in a block the
loop branches out to: (4 x loop body + rescale block) / 32.  That instantiation is what C3's timed launches run, so it
keeps its row under "bgfixed_rsq"; the level-2 prefetching loop keeps its row under "bgfixed_level2".  Each of the three
kernels also holds the two series forms of its loop (mcd_math.h: RootSeries about the chunk's centre, RootDirect in
verr^2 itself; the chunks of a verr-sorted record array whose verr^2 band is narrow): rows "..., series" and "..., direct",
and the direct loop once more with the split exponent offset (option "exp_split", BgFixedAcc::add_gs): rows "..., split".
The split loop exists once more with the quadratic series root on 32-star bands (option "root_quad", mcd_math.h: RootQuad):
rows "..., quad", 10 fused multiply-adds per term against the split rows' 11.  Its coefficients are folded once per 32
stars in a block of its own (five ds_read_b64 and four FMAs), which the count adds once per 32 terms.  The bounded quad
loop keeps its row under "bgfixed_quad_bounded".  With option "block_step" the launch runs loglike_block_kernel, the bounded
kernel whose quadratic loop takes ONE block per 32 stars for the fold, the rescale and the prefetch of a whole band (row
"..., quad, block step": 4 x loop body + that block, which is whatever the enclosing loop holds beside the 8-star body).
That loop is what nearly all of C3's chunks run, so it gives the "bgfixed" key's prefetch fields; the bounded split loop keeps
its row under "bgfixed_split_bounded", the bounded direct loop without the split under "bgfixed_direct_bounded", the bounded
delta series loop under "bgfixed_series_bounded".

"slots" prices the mix with the issue costs measured on MI355X (tools/valu_rate_probe.hip): an f64 FMA/MUL/ADD wave-
instruction = 1 slot (4 cycles on one SIMD), v_rsq/v_rcp_f64 = 2.9 slots, other VALU instructions (integer, v_ldexp,
v_frexp, moves, f32) = 0.5 slot.
"""
import hashlib
import json
import os
import re
import subprocess
import sys
from collections import Counter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mcmc_dynamics_amd", "csrc")
SOURCES = ("mcd_kernels.hip", "mcd_math.h", "mcd_exp_table.h", "mcd_internal.h", "mcd_launch.h", "mcd_dispatch.h", "mcd_chunks.h",
           "mcd_reduce.h")
SLOT_NS = 2.33

# (template tag, name, bench model key, stars per inner iteration, inner trips per outer iteration, selector
#  [, (stars, trips, selector) of the instantiation with the prefetch when its loop differs
#   [, model key of the instantiation with the prefetch when it differs]])
#   selector(Counter of the loop body) -> bool picks the loop among the kernel's innermost loops
def _sel(rsq=None, frexp=None, rcp=None, add=None, fma=None):
    def f(c):
        return ((rsq is None or c["v_rsq_f64_e32"] == rsq) and (frexp is None or c["v_frexp_mant_f64_e32"] == frexp)
                and (rcp is None or c["v_rcp_f64_e32"] == rcp) and (add is None or c["v_add_f64"] == add)
                and (fma is None or c["v_fma_f64"] + c["v_fmac_f64_e32"] == fma))
    return f


KERNELS = [
    ("ILi0ELb0EddLi1E", "CONST fixed centre", "const", 16, 1, _sel(rsq=0, rcp=1)),
    ("ILi0ELb1EddLi1E", "CONST free centre", "const_free", 8, 1, None),
    ("ILi1ELb0EddLi1E", "BGFIXED fixed centre", "bgfixed_general", 4, 1, _sel(rsq=4, frexp=4)),
    ("ILi1ELb0EddLi2E", "BGFIXED fixed, narrow", "bgfixed", 4, 2, _sel(rsq=4, frexp=0), (8, 1, _sel(rsq=8, frexp=1)),
     "bgfixed_level2"),
    ("ILi2ELb0EddLi1E", "BGGAUSS fixed centre", "bggauss_general", 4, 1, _sel(rsq=8, frexp=4)),
    ("ILi2ELb0EddLi2E", "BGGAUSS fixed, narrow", "bggauss", 4, 2, _sel(rsq=8, frexp=0)),
    ("ILi3ELb0EddLi1E", "PROFILE fixed centre", "profile_general", 8, 1, None),
    ("ILi3ELb0EddLi2E", "PROFILE fixed, narrow", "profile", 8, 1, _sel(rsq=8, rcp=1)),
    ("ILi4ELb0EddLi1E", "PROFILE_BGGAUSS fixed", "profile_bggauss", 4, 1, _sel(frexp=4)),
    ("ILi5ELb0EddLi1E", "PROFILE_BGDENS fixed", "profile_bgdens", 4, 1, _sel(frexp=4)),
    # the double Lynden-Bell models (one fast form, no narrow-range variant): PROFILE's / PROFILE_BGGAUSS's loops with the
    # second component on the shared reciprocal
    ("ILi7ELb0EddLi1E", "DOUBLE fixed centre", "double", 8, 1, None),
    ("ILi8ELb0EddLi1E", "DOUBLE_BGGAUSS fixed", "double_bggauss", 4, 1, _sel(frexp=4)),
    # the error-scale models (one fast form each): CONST's 16-star tree and PROFILE's general loop with err_scale^2 verr^2 in
    # the variance -- an FMA in place of CONST's add, one multiply more than PROFILE
    ("ILi10ELb0EddLi1E", "CONST_ESCALE fixed centre", "const_escale", 16, 1, _sel(rsq=0, rcp=1)),
    ("ILi11ELb0EddLi1E", "PROFILE_ESCALE fixed centre", "profile_escale", 8, 1, None),
    ("ILi0ELb0EffLi1E", "CONST fixed, f32", "const_f32", 16, 1, None),
    ("ILi0ELb0EfdLi1E", "CONST fixed, f32 terms f64 sums", "const_f32acc64", 16, 1, None),
    ("ILi1ELb0EffLi1E", "BGFIXED fixed, f32", "bgfixed_f32", 4, 1, None),
    ("ILi1ELb0EfdLi1E", "BGFIXED fixed, f32 terms f64 sums", "bgfixed_f32acc64", 4, 1, None),
]

# the bounded narrow-range loop (prefetching instantiation only): full tag, name, key, stars, trips, selector
BOUNDED = ("ILi1ELb0EddLi2ELb1ELi4ELb1EE", "BGFIXED fixed, narrow, prefetch, bounded", "bgfixed_rsq", 8, 4, _sel(rsq=8, frexp=0))

# the series loops of the same three kernels (mcd_math.h: RootSeries; chunks of a verr-sorted record array whose verr^2
# band is narrow): no v_rsq_f64 in the body.  Each kernel holds two of them, told apart by their v_add_f64 per term: the
# delta form (about the chunk's centre) has three -- v - v_sys, the exponent's rounding constant and delta = e - eb, which
# feeds the first FMA of the cubic -- the direct form (RootDirect: the cubic in verr^2 itself) the first two only.  The
# direct loop with the split exponent offset has two as well (v - v_sys and shifted - M): it is told from the direct loop
# without the split by its fused multiply-adds (v_fma_f64 + v_fmac_f64) per term, 11 instead of 12.
# The quadratic loops (RootQuad) are the split loops with one FMA per term fewer: 10 against 11 (the fold block, wherever
# the compiler puts it, is taken out before the selector sees the loop).
# Full tag, name, key, stars, trips, selector, prefetching, bounded [, quad]
SERIES = [
    ("ILi1ELb0EddLi2ELb0ELi4ELb0EE", "BGFIXED fixed, narrow, series", "bgfixed_series", 4, 2, _sel(rsq=0, frexp=0, add=12),
     False, False),
    ("ILi1ELb0EddLi2ELb1ELi4ELb0EE", "BGFIXED fixed, narrow, prefetch, series", "bgfixed_series", 8, 1,
     _sel(rsq=0, frexp=1, add=24), True, False),
    ("ILi1ELb0EddLi2ELb1ELi4ELb1EE", "BGFIXED fixed, narrow, prefetch, bounded, series", "bgfixed_series_bounded", 8, 4,
     _sel(rsq=0, frexp=0, add=24), True, True),
    ("ILi1ELb0EddLi2ELb0ELi4ELb0EE", "BGFIXED fixed, narrow, direct", "bgfixed_direct", 4, 2,
     _sel(rsq=0, frexp=0, add=8, fma=48), False, False),
    ("ILi1ELb0EddLi2ELb1ELi4ELb0EE", "BGFIXED fixed, narrow, prefetch, direct", "bgfixed_direct", 8, 1,
     _sel(rsq=0, frexp=1, add=16, fma=96), True, False),
    ("ILi1ELb0EddLi2ELb1ELi4ELb1EE", "BGFIXED fixed, narrow, prefetch, bounded, direct", "bgfixed_direct_bounded", 8, 4,
     _sel(rsq=0, frexp=0, add=16, fma=96), True, True),
    ("ILi1ELb0EddLi2ELb0ELi4ELb0EE", "BGFIXED fixed, narrow, split", "bgfixed_split", 4, 2,
     _sel(rsq=0, frexp=0, add=8, fma=44), False, False),
    ("ILi1ELb0EddLi2ELb1ELi4ELb0EE", "BGFIXED fixed, narrow, prefetch, split", "bgfixed_split", 8, 1,
     _sel(rsq=0, frexp=1, add=16, fma=88), True, False),
    ("ILi1ELb0EddLi2ELb1ELi4ELb1EE", "BGFIXED fixed, narrow, prefetch, bounded, split", "bgfixed_split_bounded", 8, 4,
     _sel(rsq=0, frexp=0, add=16, fma=88), True, True),
    ("ILi1ELb0EddLi2ELb0ELi4ELb0EE", "BGFIXED fixed, narrow, quad", "bgfixed_quad", 4, 2,
     _sel(rsq=0, frexp=0, add=8, fma=40), False, False, True),
    ("ILi1ELb0EddLi2ELb1ELi4ELb0EE", "BGFIXED fixed, narrow, prefetch, quad", "bgfixed_quad", 8, 1,
     _sel(rsq=0, frexp=1, add=16, fma=80), True, False, True),
    ("ILi1ELb0EddLi2ELb1ELi4ELb1EE", "BGFIXED fixed, narrow, prefetch, bounded, quad", "bgfixed_quad_bounded", 8, 4,
     _sel(rsq=0, frexp=0, add=16, fma=80), True, True, True),
]
QUAD_BLOCK = 32      # stars per fold of the quadratic loops
# what C3's timed launches run on the chunks that qualify: the "bgfixed" key's prefetch fields.  The kernel of
# option "block_step" (mcd_kernels.hip: loglike_block_kernel): name of the function, name, key, stars, selector
BLOCK_STEP = ("20loglike_block_kernelILi1ELb0EddLi4EE", "BGFIXED fixed, narrow, prefetch, bounded, quad, block step", "bgfixed", 8,
              _sel(rsq=0, frexp=0, add=16, fma=80))


def _ops(lines):
    return [l.split()[0] for l in lines if l.startswith("\t") and not l.strip().startswith((";", "."))]


def source_hash():
    h = hashlib.sha256()
    for name in SOURCES:
        with open(os.path.join(CSRC, name), "rb") as f:
            h.update(f.read())
    with open(os.path.abspath(__file__), "rb") as f:       # the extraction rules are part of what the numbers mean
        h.update(f.read())
    return h.hexdigest()[:16]


def fold_block(k, lo, hi):
    """(first, end) lines of the fold block of a quadratic loop between lines lo and hi, or None: the five ds_read_b64 in a
    row that re-read the parked coefficients, from the branch (or label) in front of them to the label or branch behind."""
    for i in range(lo, min(hi, len(k) - 5)):
        if all(k[i + j].startswith("\tds_read_b64") for j in range(5)):
            a = next(j for j in range(i, 0, -1) if re.match(r"\s*s_c?branch|^\.LBB", k[j]))
            e = next(j for j in range(i, len(k)) if re.match(r"\s*s_c?branch|^\.LBB", k[j]))
            return a + 1, e
    return None


def body_lines(k, sp):
    """the lines of loop `sp` without a fold block inside it"""
    blk = fold_block(k, sp[0], sp[1])
    if blk and blk[1] <= sp[1] + 1:
        return k[sp[0]:blk[0]] + k[blk[1]:sp[1] + 1]
    return k[sp[0]:sp[1] + 1]


def block_step_lines(k, labels, spans, best):
    """the lines of the block step of loop `best` (the 8-star body of the block-step kernel's quadratic loop): what the
    smallest loop around it holds beside it -- the fold, the rescale and the prefetch of a 32-star band -- or None"""
    around = [sp for sp in spans if sp != best and sp[0] <= best[0] and best[1] <= sp[1]]
    if not around:
        return None
    outer = min(around, key=lambda sp: sp[1] - sp[0])
    # ... and the blocks laid out behind its closing branch that jump back into it (the predicated prefetch load)
    end = outer[1] + 1
    while True:
        j = next((j for j in range(end, min(end + 24, len(k))) if re.match(r"\s*s_branch |^\.LBB", k[j])), None)
        m = re.match(r"\s*s_branch (\.LBB\d+_\d+)", k[j]) if j is not None else None
        if not (m and m.group(1) in labels and outer[0] <= labels[m.group(1)] <= outer[1]):
            break
        end = j + 1
    return k[outer[0]:best[0]] + k[best[1] + 1:end]


def rescale_block(k, labels, best, bounded, trips):
    """(first, end) lines of the rescale block of a narrow-range loop `best` (label line, closing branch line), or None.
    The 4-star loops: behind the loop's closing conditional branch, jumping back with an unconditional s_branch.  The
    bounded loop: the target of a forward branch out of the loop, closed by an s_branch back into it."""
    if bounded:
        for i in range(best[0], best[1]):
            m = re.search(r"s_cbranch_\w+ (\.LBB\d+_\d+)", k[i])
            if not (m and m.group(1) in labels and labels[m.group(1)] > best[1]):
                continue
            a0 = labels[m.group(1)]
            for j in range(a0 + 1, min(a0 + 24, len(k))):
                mb = re.match(r"\s*s_branch (\.LBB\d+_\d+)", k[j])
                if mb:
                    if mb.group(1) in labels and best[0] <= labels[mb.group(1)] <= best[1] and \
                            not any(l.startswith("\tds_read_b64") for l in k[a0:j]):      # (not the quadratic loops' fold block)
                        return a0 + 1, j
                    break
        return None
    if trips > 1:
        # the rescale block of the narrow-range loops runs on every `trips`-th iteration: it sits behind the loop's
        # closing conditional branch and jumps back with an unconditional s_branch
        for j in range(best[1] + 1, min(best[1] + 16, len(k))):
            m = re.match(r"\s*s_branch (\.LBB\d+_\d+)", k[j])
            if m:
                if m.group(1) in labels and labels[m.group(1)] <= best[1]:
                    return best[1] + 1, j
                break
    return None


def analyse(out="/tmp/isa_mix"):
    os.makedirs(out, exist_ok=True)
    subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-c",
                    os.path.join(CSRC, "mcd_kernels.hip"), "-o", os.path.join(out, "k.o"), "-save-temps=obj"],
                   check=True, capture_output=True)
    asm = open(os.path.join(out, "mcd_kernels-hip-amdgcn-amd-amdhsa-gfx950.s")).read().split("\n")
    rows = []
    # every fast kernel exists with and without the software prefetch of the next iteration's records (template
    # parameter PF, the last one of the mangled name): the main row is the instantiation without, `*_prefetch` fields and
    # a second table line give the one with
    # (the 4-wave instantiations: the combining 8- / 16-wave ones of the balanced plans run the same loops)
    # (every instantiation carries the BOUNDED parameter after WAVES: Lb0E unless it is the bounded loop)
    variants = [(row[0] + "Lb0ELi4ELb0EE", row[1], row[2], row[3], row[4], row[5], False) for row in KERNELS]
    variants += [(row[0] + "Lb1ELi4ELb0EE", row[1] + ", prefetch", row[7] if len(row) > 7 else row[2]) +
                 (row[6] if len(row) > 6 else row[3:6]) + (True,) for row in KERNELS]
    variants = [v + (False,) for v in variants]
    variants.append(BOUNDED + (True, True))
    variants += [v + (False,) * (9 - len(v)) for v in SERIES]
    variants = [v + (False,) * (9 - len(v)) for v in variants]
    variants = [("14loglike_kernel" + v[0],) + v[1:] + (False,) for v in variants]
    variants.append(BLOCK_STEP[:4] + (QUAD_BLOCK // BLOCK_STEP[3], BLOCK_STEP[4], True, True, True, True))
    for tag, name, key, per, trips, selector, with_prefetch, bounded, quad, block_step in variants:
        starts = [i for i, l in enumerate(asm) if l.startswith("_ZN3mcd12_GLOBAL__N_1" + tag)]
        if not starts:
            continue
        a = starts[0]
        e = next(i for i in range(a, len(asm)) if asm[i].startswith(".Lfunc_end"))   # kernels may have several s_endpgm
        k = asm[a:e]
        labels = {l.split(":")[0]: i for i, l in enumerate(k) if re.match(r"^\.LBB\d+_\d+:", l)}
        spans = []
        for i, l in enumerate(k):
            m = re.search(r"s_cbranch_\w+ (\.LBB\d+_\d+)", l)
            if m and m.group(1) in labels and labels[m.group(1)] < i:
                spans.append((labels[m.group(1)], i))
        inner = [sp for sp in spans if not any(o != sp and sp[0] <= o[0] and o[1] <= sp[1] for o in spans)]
        if block_step:
            # (the loop body holds no fold block and no rescale block of the other kinds: count it as it stands)
            hits = [sp for sp in sorted(inner, key=lambda sp: sp[1] - sp[0], reverse=True)
                    if selector(Counter(_ops(k[sp[0]:sp[1]]))) and sp[1] - sp[0] >= 8 * per]
            step = block_step_lines(k, labels, spans, hits[0]) if hits else None
            if step is None:
                continue
            total = Counter()
            for op, v in Counter(_ops(k[hits[0][0]:hits[0][1] + 1])).items():
                total[op] += v * trips
            for op, v in Counter(_ops(step)).items():
                total[op] += v
            rows.append(_row(name, key, with_prefetch, per * trips, total))
            continue
        ranked = sorted(inner, key=lambda sp: sp[1] - sp[0], reverse=True)
        best = None
        if selector is not None:
            # (the longest loop the selector accepts that does real work: the series loops share their kernels with short
            # copy and tail loops without a v_rsq_f64 either)
            hits = [sp for sp in ranked if selector(Counter(_ops(body_lines(k, sp)[:-1]))) and sp[1] - sp[0] >= 8 * per]
            best = hits[0] if hits else None
        if best is None:
            best = ranked[0]
        body = Counter(_ops(body_lines(k, best) if quad else k[best[0]:best[1] + 1]))
        extra = Counter()
        blk = rescale_block(k, labels, best, bounded, trips)
        if blk:
            extra = Counter(_ops(k[blk[0]:blk[1]]))
        terms = per * trips
        total = Counter()
        for op, v in body.items():
            total[op] += v * trips
        for op, v in extra.items():
            total[op] += v
        if quad:
            # per 32 terms: the loop (and its rescale block) as often as it takes, the fold block once
            fold = fold_block(k, best[0], best[1] + 120)
            if fold is None:
                continue
            for op in total:
                total[op] *= QUAD_BLOCK // terms
            terms = QUAD_BLOCK
            for op, v in Counter(_ops(k[fold[0]:fold[1]])).items():
                total[op] += v
        rows.append(_row(name, key, with_prefetch, terms, total))
    return rows


def _row(name, key, with_prefetch, terms, total):
    """one table row from the instruction tally `total` of `terms` star-walker terms"""
    def is_f64(o):
        return "f64" in o
    valu = sum(v for o, v in total.items() if o.startswith("v_"))
    f64 = sum(v for o, v in total.items() if o.startswith("v_") and is_f64(o) and not o.startswith(("v_ldexp", "v_frexp")))
    trans = sum(v for o, v in total.items() if o.startswith(("v_rsq_f64", "v_rcp_f64")))
    slots = sum(v * (2.9 if o.startswith(("v_rsq_f64", "v_rcp_f64")) else
                     1.0 if (is_f64(o) and not o.startswith(("v_ldexp", "v_frexp"))) else 0.5)
                for o, v in total.items() if o.startswith("v_"))
    return {"name": name, "model": key, "prefetch": with_prefetch, "stars_per_iteration": terms,
            "valu_per_term": valu / terms, "f64_per_term": f64 / terms, "trans_f64_per_term": trans / terms,
            "other_per_term": (valu - f64) / terms, "slots_per_term": slots / terms,
            "lds_per_term": sum(v for o, v in total.items() if o.startswith("ds_")) / terms,
            "salu_smem_per_term": sum(v for o, v in total.items() if o.startswith("s_")) / terms}


def merge_variants(rows):
    """{model: row of the instantiation without prefetch + `<field>_prefetch` for the one with}"""
    out = {r["model"]: dict(r) for r in rows if not r["prefetch"]}
    for r in rows:
        if r["prefetch"] and r["model"] not in out:          # (a prefetch-only row: bgfixed_level2)
            out[r["model"]] = dict(r)
        if r["prefetch"]:
            for k in ("valu_per_term", "f64_per_term", "other_per_term", "slots_per_term", "salu_smem_per_term"):
                out[r["model"]][k + "_prefetch"] = r[k]
    for r in out.values():
        del r["prefetch"]
    return out


def main():
    rows = analyse()
    print("{0:34s} {1:>9s} {2:>8s} {3:>8s} {4:>10s} {5:>14s}".format("kernel (fast path)", "VALU/term", "f64", "other",
                                                                    "slots/term", "predicted us"))
    for r in rows:
        pred = r["slots_per_term"] * SLOT_NS * (2.56e8 / 64) / 1024 * 1e-3
        print("{0:34s} {1:9.2f} {2:8.2f} {3:8.2f} {4:10.2f} {5:14.1f}".format(r["name"], r["valu_per_term"], r["f64_per_term"],
                                                                           r["other_per_term"], r["slots_per_term"], pred))
    if len(sys.argv) == 3 and sys.argv[1] == "--json":
        merged = merge_variants(rows)
        # what the second Lynden-Bell component adds to PROFILE's loop per term (tests/test_double_isa_cpu.py holds the margin)
        double_note = {
            "valu_per_term_over_profile": merged["double"]["valu_per_term"] - merged["profile_general"]["valu_per_term"],
            "valu_per_term_over_profile_bggauss": merged["double_bggauss"]["valu_per_term"] - merged["profile_bggauss"]["valu_per_term"],
            "trans_f64_per_term_over_profile": merged["double"]["trans_f64_per_term"] - merged["profile_general"]["trans_f64_per_term"],
            "margin": 7.0,
            "listing": "per term: 1 v_add_f64 (m_2 = rho_2^2 + r^2), 4 v_mul_f64 (v_maxy_c dx, m_1 m_2, K_2 cross_2, its "
                       "product with m_1; K_1 cross_1 takes the place of PROFILE's K_1 inv), 2 v_fma_f64 (the second cross, "
                       "the numerator); no second v_rcp_f64 sequence",
        } if "double" in merged and "double_bggauss" in merged else None
        # what err_scale^2 adds to the base models' loops per term (tests/test_escale_cpu.py holds the margin)
        escale_note = {
            "valu_per_term_over_const": merged["const_escale"]["valu_per_term"] - merged["const"]["valu_per_term"],
            "valu_per_term_over_profile": merged["profile_escale"]["valu_per_term"] - merged["profile_general"]["valu_per_term"],
            "margin": 1.0,
            "listing": "per term: CONST v_fma_f64 (err_scale^2 verr^2 + sigma_max^2) in place of v_add_f64; PROFILE one "
                       "v_mul_f64 (err_scale^2 verr^2) in front of the variance's v_fma_f64",
        } if "const_escale" in merged and "profile_escale" in merged else None
        with open(sys.argv[2], "w") as f:
            json.dump({"source_sha16": source_hash(), "generated_by": "tools/isa_mix.py", "double_models": double_note,
                       "escale_models": escale_note,
                       "note": "VALU wave-instructions per star-walker term in the hot loop nest of mcd::loglike_kernel "
                               "(gfx950 ISA from hipcc -save-temps); prologue, final log and tails not included",
                       "kernels": merged}, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    sys.exit(main())
