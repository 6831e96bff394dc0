#!/usr/bin/env python3
"""Generates image-text-retrieval_amd/csrc/scan_mainloop_asm.inc: the fp32 main loop of the SCAN kernel as ONE inline-asm
statement with hand-allocated registers.

Why assembly.  The loop issues its global loads two chunks ahead and counts them with its own s_waitcnt vmcnt(N) (hipcc's
bookkeeping exposed a full memory latency per chunk).  A load hipcc cannot see has, to hipcc, a destination that is
"written" when the asm statement ends: with compiler-allocated stage registers the allocator is free to copy, spill or reuse
them while data is in flight, and at this kernel's register budget every restructuring of the loop made it do so
(tools/audit_asm_loads.py).  Here every register the loop touches is named literally and listed as clobbered, so hipcc
keeps its own values out of them for the whole statement, nothing is in flight when the statement ends (the last wait is
vmcnt(0)), and the instruction interleave is exactly the one written below instead of a scheduler's best effort.

Loop structure (per 32-wide K chunk kc, 72 x v_mfma_f32_16x16x4_f32 per wave).  Chunk c lives in LDS buffer
c % 2 and, before that, in register stage A (c even) or B (c odd):
    first half    s_waitcnt lgkmcnt(0): the F0(kc) fragments read during the previous half have landed
                  36 MFMAs on F0(kc), one memory instruction behind each of the first 24:
                  s_waitcnt vmcnt(7), then park chunk kc+1 in the other buffer (7 ds_write_b128) ALTERNATING with the reads of
                  fragment set F1(kc) (10 ds_read_b128), then refill that stage with chunk kc+3 (7 global loads)
    s_waitcnt lgkmcnt(0); s_barrier        (chunk kc+1 visible; every wave done reading chunk kc)
    second half   36 MFMAs on F1(kc); behind the first 10: read F0(kc+1) from the other buffer
The stores alternate with the reads because four waves that issue 16-byte LDS stores behind CONSECUTIVE MFMAs outrun the LDS
(one ds_write_b128 keeps it busy ~13 cycles, the four waves of a workgroup leave the same barrier, a slot is 32 cycles): the
in-order wave waits at the store, and a wave that is alone on its SIMD -- the other workgroup of the CU is in its epilogue --
has nobody to fill the MFMA slots it misses.  SCHEDULES below keeps every placement that was measured
(tools/ubench/mfma_pipe.hip runs each of them; table in profiles/scan_lone/README.md), among them parking chunk kc+2 one half
chunk earlier (`early`), which is faster in the micro-benchmark and not in the kernel.
The last three chunks take no refill; the very last parks nothing.  Then the accumulators are parked transposed in LDS.

Schedule rules (verify() below walks every entry path and checks them; tests/test_scan_mainloop_paths_gpu.py runs it):
  * A store into buffer X for chunk c+1 is issued after the barrier that follows every wave's last read of chunk c-1 from X,
    and it is complete (lgkmcnt(0)) before the barrier that precedes the first read of chunk c+1.
  * The vmcnt wait sits in front of the first store that reads a stage register; the loads issued after that stage's are the
    7 of the other stage (vmcnt(7)), or none in the tail (vmcnt(0)).  The refill loads of a stage follow its last store.
  * LDS operations of one wave complete in order, so the wait at the top of a chunk may be counted: lgkmcnt(number of park
    stores issued behind the F0 reads; none in the committed schedule).  There is no scalar memory instruction in the statement.
  * The MFMA sequence per accumulator is fixed (chunk, F0 then F1, component-major): scores do not depend on the schedule.
  * A stand-alone 4-byte s_waitcnt that a schedule adds is paired with an s_nop 0, so every schedule differs from every other
    by a multiple of 8 bytes at every point of the stream (a uniform shift of 4 mod 8 bytes changes the timing of a
    hand-written stream by itself).

    python tools/gen_scan_mainloop.py            # rewrite the .inc
    python tools/gen_scan_mainloop.py --check    # exit 1 if the committed .inc differs from what this script generates
    python tools/gen_scan_mainloop.py --verify   # walk every legal schedule along every entry path (verify())
    python tools/gen_scan_mainloop.py --ubench DIR               # one .inc per schedule for tools/ubench/mfma_pipe.hip
    python tools/gen_scan_mainloop.py --schedule NAME --out FILE # one schedule, e.g. into a side-by-side tree (tools/ab/)
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "image-text-retrieval_amd", "csrc", "scan_mainloop_asm.inc")

# ---- geometry (scan_common.h)
SC_MT, SC_NT, SC_MTILES = 144, 64, 9
SC_ROWS, SC_PLANES = SC_MT + SC_NT + 16, 8
STAGE_BYTES = SC_PLANES * SC_ROWS * 16          # 28 672: one LDS operand buffer
SC_LDT = SC_MT + 4                              # row stride (floats) of the parked block [column][row]

# ---- register map (VGPRs 64..235 and SGPRs 80..86 belong to the statement)
ACC0, F0A, F0B, F1A, F1B, STA, STB = 64, 100, 136, 140, 176, 180, 208
V_LO, V_HI = 64, 235
S_PA, S_PB, S_PB2, S_N = 80, 82, 84, 86


def vr(base, n=4):
    return "v[%d:%d]" % (base, base + n - 1)


def acc(m):
    return vr(ACC0 + 4 * m)


def stage(P, i):
    return vr((STA if P == 'A' else STB) + 4 * i)


def lstore(P, buf):
    """7 x ds_write_b128: stage P -> LDS buffer `buf` (plane / XOR layout; pass c of rows = la0 + 16 c, see scan_mainloop.inc)."""
    o = buf * STAGE_BYTES
    return ["ds_write_b128 %%[la0], %s offset:%d" % (stage(P, 0), o),
            "ds_write_b128 %%[la0], %s offset:%d" % (stage(P, 1), o + 32 * 16),
            "ds_write_b128 %%[la0], %s offset:%d" % (stage(P, 2), o + 64 * 16),
            "ds_write_b128 %%[la0], %s offset:%d" % (stage(P, 3), o + 96 * 16),
            "ds_write_b128 %%[la4], %s offset:%d" % (stage(P, 4), o),
            "ds_write_b128 %%[la0], %s offset:%d" % (stage(P, 5), o + SC_MT * 16),
            "ds_write_b128 %%[la0], %s offset:%d" % (stage(P, 6), o + (SC_MT + 32) * 16)]


def gload(P):
    """7 x global_load_dwordx4 of the chunk the running pointers address, then advance the pointers by one chunk (128 B)."""
    ins = ["global_load_dwordx4 %s, %%[va%d], s[%d:%d]" % (stage(P, i), i, S_PA, S_PA + 1) for i in range(5)]
    ins.append("global_load_dwordx4 %s, %%[vb0], s[%d:%d]" % (stage(P, 5), S_PB, S_PB + 1))
    ins.append("global_load_dwordx4 %s, %%[vb0], s[%d:%d]" % (stage(P, 6), S_PB2, S_PB2 + 1))
    adv = []
    for s in (S_PA, S_PB, S_PB2):
        adv += ["s_add_u32 s%d, s%d, 128" % (s, s), "s_addc_u32 s%d, s%d, 0" % (s + 1, s + 1)]
    return ins, adv


def fread(which, buf):
    """10 x ds_read_b128: fragment set F0 (k-planes 0..3) or F1 (planes 4..7) of the chunk in LDS buffer `buf`."""
    fa, fb, ra, rb = (F0A, F0B, "ra0", "rb0") if which == 0 else (F1A, F1B, "ra1", "rb1")
    o = buf * STAGE_BYTES
    return ["ds_read_b128 %s, %%[%s] offset:%d" % (vr(fb), rb, o)] + \
           ["ds_read_b128 %s, %%[%s] offset:%d" % (vr(fa + 4 * m), ra, o + m * 256) for m in range(SC_MTILES)]


def mfmas(which):
    """36 MFMAs of one fragment set, component-major (consecutive MFMAs hit different accumulators)."""
    fa, fb = (F0A, F0B) if which == 0 else (F1A, F1B)
    return ["v_mfma_f32_16x16x4_f32 %s, v%d, v%d, %s" % (acc(m), fa + 4 * m + c, fb + c, acc(m))
            for c in range(4) for m in range(SC_MTILES)]


class Sched:
    """Where the memory instructions of a chunk sit between its MFMAs.

    early    how many of the 7 ds_write_b128 that park chunk kc+2 are issued in the SECOND half of chunk kc (behind the F0
             reads of that half); the other 7 - early stay in the first half of chunk kc+1.  0 = all in the first half.
    h1_order order of the first half's memory instructions: W (park stores), G (refill loads, always after W), R (F1 fragment
             reads); "WGR" = the groups one after the other, a longer string names every instruction ("GRGR...")
    h1_span, h2_span   0: one instruction behind each of the first MFMAs of the half; n > 0: spread evenly over the first n slots
    h2_slots explicit slots of the second half's instructions (10 reads, then the early stores) instead of h2_span
    sepwait  the chunk opens with a counted lgkmcnt only; the vmcnt wait sits in front of the first store that reads a stage
             register (False: one combined wait at the top of the chunk)
    barrier / drain   micro-benchmark only (tools/ubench/mfma_pipe.hip): leave out the s_barrier / the lgkmcnt(0) in front of
             it to see what each costs.  Such a schedule is racy and is refused as the committed one."""

    def __init__(self, early=0, h1_order="WGR", h1_span=0, h2_span=0, sepwait=False, barrier=True, drain=True, h2_slots=None):
        assert 0 <= early <= 7 and set(h1_order) == set("WGR") and h1_order.rindex("W") < h1_order.index("G")
        self.h2_slots = h2_slots
        assert sepwait or early == 0, "a store in the second half needs its own vmcnt wait"
        self.early, self.h1_order, self.h1_span, self.h2_span = early, h1_order, h1_span, h2_span
        self.sepwait, self.barrier, self.drain = sepwait, barrier, drain

    @property
    def legal(self):
        return self.barrier and self.drain


# The schedules the micro-benchmark compares (python tools/gen_scan_mainloop.py --ubench DIR); COMMITTED is the kernel's.
SCHEDULES = {
    "parent":        Sched(),                                                      # all 17 LDS + 7 global behind MFMAs 0..23 / 10 reads behind 0..9
    "nobarrier":     Sched(barrier=False),                                         # attribution: racy
    "nodrain":       Sched(drain=False),                                           # attribution: racy
    "sepwait":       Sched(sepwait=True, h1_order="RWG"),                          # F1 reads first, vmcnt wait 10 MFMAs later
    "spread":        Sched(h1_span=36, h2_span=30),                                # parent's order, spread over the half
    "early7":        Sched(early=7, sepwait=True, h1_order="WGR"),                 # whole park one half earlier, slots 0..16 of each half
    "early7_rg":     Sched(early=7, sepwait=True, h1_order="WRG"),
    "early7_spread": Sched(early=7, sepwait=True, h1_order="WRG", h1_span=32, h2_span=32),
    "early7_h1spr":  Sched(early=7, sepwait=True, h1_order="WRG", h1_span=32),
    "early7_h2spr":  Sched(early=7, sepwait=True, h1_order="WRG", h2_span=32),
    "early5_spread": Sched(early=5, sepwait=True, h1_order="WRG", h1_span=32, h2_span=30),
    "e7_s36":        Sched(early=7, sepwait=True, h1_order="WRG", h1_span=36, h2_span=36),
    "e7_s28":        Sched(early=7, sepwait=True, h1_order="WRG", h1_span=28, h2_span=28),
    "e7_gr":         Sched(early=7, sepwait=True, h1_order="WGR", h1_span=32, h2_span=32),
    "e7_alt":        Sched(early=7, sepwait=True, h1_order="W" * 7 + "RG" * 7 + "RRR", h1_span=32, h2_span=32),
    "e7_w2":         Sched(early=7, sepwait=True, h1_order="WRG", h1_span=32, h2_slots=list(range(10)) + list(range(11, 24, 2))),
    "e7_w3":         Sched(early=7, sepwait=True, h1_order="WRG", h1_span=32, h2_slots=list(range(10)) + list(range(12, 31, 3))),
    "e7_w4":         Sched(early=7, sepwait=True, h1_order="WRG", h1_span=32, h2_slots=list(range(10)) + list(range(10, 35, 4))),
    "e7_r2w3":       Sched(early=7, sepwait=True, h1_order="WRG", h1_span=32, h2_slots=list(range(0, 15, 2)) + [15, 16] + list(range(17, 36, 3))),
    "e0_w2":         Sched(sepwait=True, h1_order="WR" * 7 + "RRR" + "G" * 7),     # parent's window; a store behind every other MFMA, reads between
    "e0_w2c":        Sched(h1_order="WR" * 7 + "RRR" + "G" * 7),                   # the same with the parent's combined wait
    "e0_w2s":        Sched(sepwait=True, h1_order="WR" * 7 + "RRR" + "G" * 7, h2_span=20),
    "early4":        Sched(early=4, sepwait=True, h1_order="WRG"),
    "early4_spread": Sched(early=4, sepwait=True, h1_order="WRG", h1_span=32, h2_span=28),
    "early3_spread": Sched(early=3, sepwait=True, h1_order="WRG", h1_span=32, h2_span=26),
}
COMMITTED = "e0_w2"

N_SLOTS = 36
VMWAIT_PAD = "s_nop 0"      # a stand-alone 4-byte wait gets a 4-byte partner: the statement grows in steps of 8 bytes (see the docstring)


def slot_of(n, span):
    """MFMA index behind which the i-th of n memory instructions of a half is placed."""
    if span == 0:
        return list(range(n))
    assert n <= span <= N_SLOTS
    return [(i * span) // n for i in range(n)]


def interleave(mf, mem, span, adv=(), slots=None):
    """mem: list of instruction groups (one slot each); adv: scalar pointer updates, one per free slot after the last group."""
    pos = list(slots[:len(mem)]) if slots else slot_of(len(mem), span)
    assert pos == sorted(pos) and (not pos or pos[-1] < N_SLOTS)
    at = dict(zip(pos, mem))
    assert len(at) == len(mem)
    adv = list(adv)
    out = []
    for i, x in enumerate(mf):
        out.append(x)
        if i in at:
            out += at[i]
        elif adv and (not pos or i > pos[-1]):
            out.append(adv.pop(0))
    return out + adv


def chunk(P, cur, nxt, park2, load, sc):
    """One steady-state / tail chunk kc.  P: the stage that holds chunk kc+1 (the other one, Q, holds chunk kc+2 if there is
    one: park2); cur / nxt: LDS buffers of chunk kc / kc+1; load: there is a chunk kc+3 to refill P with."""
    Q = 'B' if P == 'A' else 'A'
    vm_top = 7 if park2 else 0                # loads issued after stage P's: those of chunk kc+2
    # F0(kc) was read in the previous half, followed there by `early` park stores (LDS operations of a wave complete in order)
    if sc.sepwait:
        ins = ["s_waitcnt lgkmcnt(%d)" % sc.early]
    else:
        ins = ["s_waitcnt vmcnt(%d) lgkmcnt(0)" % vm_top]
    groups = {"W": [[x] for x in lstore(P, nxt)[sc.early:]], "G": [], "R": [[x] for x in fread(1, cur)]}
    if sc.sepwait and sc.early == 0:
        groups["W"][0] = ["s_waitcnt vmcnt(%d)" % vm_top, VMWAIT_PAD] + groups["W"][0]
    adv = []
    if load:
        ld, adv = gload(P)
        groups["G"] = [[x] for x in ld]
    if len(sc.h1_order) == 3:
        mem = [g for k in sc.h1_order for g in groups[k]]
    else:                                     # instruction by instruction; a group that is absent in this chunk is skipped
        mem = [groups[k].pop(0) for k in sc.h1_order if groups[k]]
        assert not any(groups.values())
    ins += interleave(mfmas(0), mem, sc.h1_span, adv)
    ins += (["s_waitcnt lgkmcnt(0)"] if sc.drain else ["s_nop 0"]) + (["s_barrier"] if sc.barrier else ["s_nop 0"])
    mem2 = [[x] for x in fread(0, nxt)]
    if park2 and sc.early:
        w = [[x] for x in lstore(Q, cur)[:sc.early]]
        w[0] = ["s_waitcnt vmcnt(%d)" % (7 if load else 0), VMWAIT_PAD] + w[0]     # loads issued after stage Q's: the refill just above
        mem2 += w
    ins += interleave(mfmas(1), mem2, sc.h2_span, slots=sc.h2_slots)
    return ins


def last(cur):
    ins = ["s_waitcnt lgkmcnt(0)"]
    mem = fread(1, cur)
    for i, x in enumerate(mfmas(0)):
        ins.append(x)
        if i < len(mem):
            ins.append(mem[i])
    ins.append("s_waitcnt lgkmcnt(0)")
    ins += mfmas(1)
    return ins


def program(sc):
    L = lambda name: ".Lscan_%s_%%=" % name          # %= : unique per asm statement instance
    ins = []
    ins += ["s_mov_b64 s[%d:%d], %%[abase]" % (S_PA, S_PA + 1), "s_mov_b64 s[%d:%d], %%[bbase]" % (S_PB, S_PB + 1),
            "s_mov_b64 s[%d:%d], %%[bbase2]" % (S_PB2, S_PB2 + 1), "s_mov_b32 s%d, %%[nmain]" % S_N]
    ins += ["v_mov_b32 v%d, 0" % r for r in range(ACC0, ACC0 + 4 * SC_MTILES)]
    # prologue: chunk 0 -> LDS buffer 0, stage B = chunk 1, stage A = chunk 2
    for P in ('A', 'B'):
        ld, adv = gload(P)
        ins += ld + adv
    ins += ["s_waitcnt vmcnt(7)"] + lstore('A', 0)
    ld, adv = gload('A')
    ins += ld + adv
    ins += ["s_waitcnt lgkmcnt(0)", "s_barrier"] + fread(0, 0)
    if sc.early:                                      # what the second half of a chunk "-1" would have parked: chunk 1, behind the F0 reads
        ins += ["s_waitcnt vmcnt(7)", VMWAIT_PAD] + lstore('B', 1)[:sc.early]
    # steady state: chunks 0 .. nk-4; s86 counts the chunks left that still have a chunk kc+3 to fetch
    ins += [L("loop") + ":",
            "s_cmp_lt_i32 s%d, 1" % S_N, "s_cbranch_scc1 " + L("tail_even")]
    ins += chunk('B', 0, 1, True, True, sc)
    ins += ["s_sub_u32 s%d, s%d, 1" % (S_N, S_N), "s_cmp_lt_i32 s%d, 1" % S_N, "s_cbranch_scc1 " + L("tail_odd")]
    ins += chunk('A', 1, 0, True, True, sc)
    ins += ["s_sub_u32 s%d, s%d, 1" % (S_N, S_N), "s_branch " + L("loop")]
    # peeled tails: chunks nk-3, nk-2 (no refill; the last vmcnt wait drains everything), nk-1
    ins += [L("tail_even") + ":"] + chunk('B', 0, 1, True, False, sc) + chunk('A', 1, 0, False, False, sc) + last(0) + ["s_branch " + L("done")]
    ins += [L("tail_odd") + ":"] + chunk('A', 1, 0, True, False, sc) + chunk('B', 0, 1, False, False, sc) + last(1)
    ins += [L("done") + ":"]
    # park the 144 x 64 block transposed: arawt[column][row]; the staging buffers alias it, so every wave must be done reading
    ins += ["s_nop 15", "s_nop 3", "s_barrier"]               # MFMA results readable (8-pass XDL -> LDS data read), all F reads done
    ins += ["ds_write_b128 %%[park], %s offset:%d" % (acc(m), m * 64) for m in range(SC_MTILES)]
    ins += ["s_waitcnt lgkmcnt(0)", "s_barrier"]
    return ins


def verify(sc, nks=range(3, 12)):
    """Walks the statement one wave at a time, along every entry path (nk = 3 .. 11 chunks), and checks the schedule rules:
      * a register is read (ds_write data, MFMA operand) only after the wait that retires its load / LDS read, counted in order;
      * a ds_write into LDS buffer X is issued after a barrier that follows the retirement of every earlier read from X, and a
        read from X sees a complete chunk whose 7 stores were retired before a barrier (every wave runs this same stream, so a
        barrier that follows this wave's retirement follows every wave's);
      * each stage item is parked exactly where lstore() puts it, each chunk is fetched once and never past nk - 1;
      * every accumulator sees chunk 0 .. nk-1, F0 then F1, components 0 .. 3: the MFMA order of the parent;
      * nothing is in flight at the end.
    Returns the number of instructions walked; raises AssertionError with the position otherwise."""
    import re
    prog = program(sc)
    labels = {x[:-1]: i for i, x in enumerate(prog) if x.endswith(":")}
    st_item = {}
    for P in "AB":
        for i, x in enumerate(lstore(P, 0)):
            m = re.match(r"ds_write_b128 %\[(\w+)\], v\[(\d+):\d+\] offset:(\d+)", x)
            st_item[int(m.group(2))] = (P, i, m.group(1), int(m.group(3)))
    fr_item = {}
    for w in (0, 1):
        for x in fread(w, 0):
            m = re.match(r"ds_read_b128 v\[(\d+):\d+\], %\[(\w+)\] offset:(\d+)", x)
            fr_item[int(m.group(1))] = (w, m.group(2), int(m.group(3)))
    walked = 0
    for nk in nks:
        sreg = {S_N: nk - 3}
        ptr = {S_PA: 0, S_PB: 0, S_PB2: 0}
        scc, pc = False, 0
        vm, lg = [], []                              # in flight, oldest first
        val = {}                                     # base VGPR -> what it holds
        inflight = set()
        lds = [{}, {}]                               # buffer -> {stage item: chunk}
        rd_open, wr_open = [False, False], [False, False]
        seq = {m: [] for m in range(SC_MTILES)}
        fetched = []

        def retire(q, n):
            while len(q) > n:
                kind, reg, what = q.pop(0)
                inflight.discard(reg)
                if kind == "load" or kind == "read":
                    val[reg] = what

        while pc < len(prog):
            x = prog[pc]
            where = "nk=%d, instruction %d `%s`" % (nk, pc, x)
            pc += 1
            walked += 1
            op = x.split()[0]
            if x.endswith(":") or op in ("s_nop", "s_mov_b64", "s_mov_b32", "v_mov_b32", "s_addc_u32"):
                continue
            if op == "s_add_u32":
                ptr[int(re.match(r"s_add_u32 s(\d+)", x).group(1))] += 1
            elif op == "s_sub_u32":
                sreg[S_N] -= 1
            elif op == "s_cmp_lt_i32":
                scc = sreg[S_N] < 1
            elif op == "s_cbranch_scc1":
                if scc:
                    pc = labels[x.split()[1]]
            elif op == "s_branch":
                pc = labels[x.split()[1]]
            elif op == "global_load_dwordx4":
                m = re.match(r"global_load_dwordx4 v\[(\d+):\d+\], %\[\w+\], s\[(\d+):", x)
                reg, c = int(m.group(1)), ptr[int(m.group(2))]
                P, i = st_item[reg][:2]
                assert c < nk, "fetch past the last chunk: " + where
                assert reg not in inflight, "stage register reloaded in flight: " + where
                assert val.get(reg) is None, "stage register reloaded before it was parked: " + where
                fetched.append((c, i))
                inflight.add(reg)
                vm.append(("load", reg, (c, i)))
            elif op == "ds_write_b128" and "%[park]" not in x:
                m = re.match(r"ds_write_b128 %\[(\w+)\], v\[(\d+):\d+\] offset:(\d+)", x)
                reg, off = int(m.group(2)), int(m.group(3))
                P, i, addr, o0 = st_item[reg]
                buf = off // STAGE_BYTES
                assert m.group(1) == addr and off - buf * STAGE_BYTES == o0, "store to the wrong place: " + where
                assert reg not in inflight and val.get(reg) is not None, "store of a stage register that has not landed: " + where
                c = val[reg][0]
                assert buf == c % 2 and val[reg][1] == i, "chunk parked in the wrong buffer: " + where
                assert not rd_open[buf], "store into a buffer other waves may still read: " + where
                val[reg] = None
                lds[buf][i] = ("pending", c)
                wr_open[buf] = True
                lg.append(("write", (buf, i), c))
            elif op == "ds_write_b128":
                assert not [q for q in lg if q[0] != "park"] and not vm and not any(rd_open), "park with something in flight: " + where
                lg.append(("park", None, None))
            elif op == "ds_read_b128":
                m = re.match(r"ds_read_b128 v\[(\d+):\d+\], %\[(\w+)\] offset:(\d+)", x)
                reg, off = int(m.group(1)), int(m.group(3))
                w, addr, o0 = fr_item[reg]
                buf = off // STAGE_BYTES
                assert m.group(2) == addr and off - buf * STAGE_BYTES == o0, "read from the wrong place: " + where
                cs = set(lds[buf].get(i) for i in range(7))
                assert len(cs) == 1 and None not in cs and not wr_open[buf], "read of a buffer that is not complete and visible: " + where
                rd_open[buf] = True
                inflight.add(reg)
                lg.append(("read", reg, (cs.pop(), w, buf)))
            elif op == "s_waitcnt":
                m = re.search(r"vmcnt\((\d+)\)", x)
                if m:
                    retire(vm, int(m.group(1)))
                m = re.search(r"lgkmcnt\((\d+)\)", x)
                if m:
                    n = int(m.group(1))
                    while len(lg) > n:
                        kind, reg, what = lg.pop(0)
                        if kind == "read":
                            inflight.discard(reg)
                            val[reg] = what
                        elif kind == "write":
                            lds[reg[0]][reg[1]] = what
            elif op == "s_barrier":
                for b in (0, 1):
                    if not any(k == "read" and w[2] == b for k, r, w in lg):
                        rd_open[b] = False
                    if not any(k == "write" and r[0] == b for k, r, w in lg):
                        wr_open[b] = False
            elif op == "v_mfma_f32_16x16x4_f32":
                m = re.match(r"v_mfma_f32_16x16x4_f32 v\[(\d+):\d+\], v(\d+), v(\d+), v\[(\d+):", x)
                d, a_, b_ = int(m.group(1)), int(m.group(2)), int(m.group(3))
                assert d == int(m.group(4))
                mt = (d - ACC0) // 4
                which = 0 if a_ < F0B else 1
                fa, fb = (F0A, F0B) if which == 0 else (F1A, F1B)
                comp = b_ - fb
                ra_ = fa + 4 * mt
                assert a_ == ra_ + comp and 0 <= comp < 4, "operand pairing: " + where
                for r in (ra_, fb):
                    assert r not in inflight and val.get(r) is not None, "MFMA on a fragment that has not landed: " + where
                assert val[ra_][:2] == val[fb][:2] and val[ra_][1] == which, "fragments of two chunks: " + where
                seq[mt].append((val[ra_][0], which, comp))
            else:
                raise AssertionError("unknown instruction: " + where)
        assert not vm and not lg and not inflight, "in flight at the end (nk=%d): %r %r" % (nk, vm, lg)
        want = [(c, w, k) for c in range(nk) for w in (0, 1) for k in range(4)]
        for mt in range(SC_MTILES):
            assert seq[mt] == want, "MFMA order of accumulator %d changed (nk=%d)" % (mt, nk)
        assert sorted(fetched) == [(c, i) for c in range(nk) for i in range(7)], "chunks fetched (nk=%d)" % nk
    return walked


def render(sc=None):
    ins = program(sc or SCHEDULES[COMMITTED])
    lines = []
    lines.append("// GENERATED by tools/gen_scan_mainloop.py -- do not edit; regenerate and commit (tests/test_isa_audit.py checks it is current).")
    lines.append("// One asm statement = prologue + K loop + peeled tail + park of scan_xattn_body<0>; register map and rationale in the generator.")
    lines.append("    asm volatile(")
    for x in ins:
        lines.append('        "%s\\n\\t"' % x)
    lines.append("        :")
    lines.append('        : [va0] "v"(va0), [va1] "v"(va1), [va2] "v"(va2), [va3] "v"(va3), [va4] "v"(va4), [vb0] "v"(vb0), [la0] "v"(la0), [la4] "v"(la4),')
    lines.append('          [ra0] "v"(ra0), [ra1] "v"(ra1), [rb0] "v"(rb0), [rb1] "v"(rb1), [park] "v"(park_addr),')
    lines.append('          [abase] "s"(abase), [bbase] "s"(bbase), [bbase2] "s"(bbase2), [nmain] "s"(nmain)')
    clob = ['"memory"', '"scc"'] + ['"s%d"' % s for s in range(S_PA, S_N + 1)] + ['"v%d"' % r for r in range(V_LO, V_HI + 1)]
    row, rows = [], []
    for c in clob:
        row.append(c)
        if len(row) == 16:
            rows.append(", ".join(row))
            row = []
    if row:
        rows.append(", ".join(row))
    lines.append("        : " + (",\n          ".join(rows)) + ");")
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    if "--verify" in sys.argv:
        for name, sc in SCHEDULES.items():
            if sc.legal:
                print("%-14s ok, %d instructions walked" % (name, verify(sc)))
        sys.exit(0)
    if "--ubench" in sys.argv:                       # one .inc per schedule, for tools/ubench/mfma_pipe.hip (not committed)
        d = sys.argv[sys.argv.index("--ubench") + 1]
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, "schedules.h"), "w") as f:
            f.write("#ifdef SCHED_BODY\n")
            for i, name in enumerate(SCHEDULES):
                open(os.path.join(d, "sched_%s.inc" % name), "w").write(render(SCHEDULES[name]))
                f.write('if constexpr (V == %d) {\n#include "sched_%s.inc"\n}\n' % (i, name))
            f.write("#endif\n#ifdef SCHED_LIST\n")
            for i, name in enumerate(SCHEDULES):
                f.write('SCHED(%d, "%s%s")\n' % (i, name, "" if SCHEDULES[name].legal else " (racy: timing only)"))
            f.write("#endif\n")
        sys.exit(0)
    name, out = COMMITTED, OUT
    if "--schedule" in sys.argv:                     # another legal schedule, into a side-by-side tree for an A/B run (--out FILE)
        name = sys.argv[sys.argv.index("--schedule") + 1]
        out = sys.argv[sys.argv.index("--out") + 1]
    assert SCHEDULES[name].legal
    verify(SCHEDULES[name])
    text = render(SCHEDULES[name])
    if "--check" in sys.argv:
        cur = open(out).read() if os.path.exists(out) else ""
        sys.exit(0 if cur == text else 1)
    open(out, "w").write(text)
    n_mfma = text.count("v_mfma")
    print("wrote %s: %d lines, %d MFMAs (= 8 chunk bodies x 72 - the last-chunk halves)" % (out, text.count("\n"), n_mfma))
