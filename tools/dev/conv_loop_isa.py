#!/usr/bin/env python
"""Main loop of conv3x3_split_kernel in the compiler's assembly, counted per instantiation (development aid).

    hipcc <the Makefile's FLAGS> --cuda-device-only -S csrc/conv.hip -o conv.s && python tools/dev/conv_loop_isa.py conv.s

Per instantiation: the kernel descriptor's figures (VGPRs, SGPRs, scratch bytes, LDS bytes) and, for one iteration of the chunk
loop (the loop with the most MFMAs): MFMAs, LDS reads and writes, `s_waitcnt lgkmcnt` waits, how many of them drain the queue
(lgkmcnt(0)), how many drain it between two MFMAs with no barrier between, and how many waits stand within three instructions of
the LDS read they wait for (a round trip nothing covers).  With --taps: the instruction classes in order, one line per run between MFMAs."""
import re
import sys


def template_args(name):
    m = re.search(r"conv3x3_split_kernelI((?:L[ib]\d+E)+)E", name)
    if not m:
        return name
    args = re.findall(r"L([ib])(\d+)E", m.group(1))
    return "<" + ",".join(v if t == "i" else ("true" if v == "1" else "false") for t, v in args) + ">"


def functions(lines):
    cur, body = None, []
    for ln in lines:
        m = re.match(r"^(_Z\w*conv3x3_split_kernel\w*):", ln)
        if m:
            cur, body = m.group(1), []
            continue
        if cur is not None:
            body.append(ln)
            if ln.startswith(".Lfunc_end"):
                yield cur, body
                cur = None


def meta(lines, name):
    out = {}
    txt = "".join(lines)
    i = txt.find(f".amdhsa_kernel {name}")
    blk = txt[i: txt.find(".end_amdhsa_kernel", i)]
    for key in ("next_free_vgpr", "accum_offset", "next_free_sgpr", "private_segment_fixed_size", "group_segment_fixed_size"):
        m = re.search(rf"\.amdhsa_{key} (\d+)", blk)
        out[key] = int(m.group(1)) if m else None
    return out


def main_loop(body):
    ins = [ln.strip() for ln in body if ln.strip() and not ln.strip().startswith(";")]
    labels = {m.group(1): i for i, ln in enumerate(ins) if (m := re.match(r"^(\.LBB\d+_\d+):", ln))}
    best = None
    for i, ln in enumerate(ins):
        m = re.match(r"^s_cbranch_\w+ (\.LBB\d+_\d+)", ln) or re.match(r"^s_branch (\.LBB\d+_\d+)", ln)
        if m and m.group(1) in labels and labels[m.group(1)] < i:
            seg = [x for x in ins[labels[m.group(1)]: i + 1] if not x.startswith(".")]
            n = sum(x.startswith("v_mfma") for x in seg)
            if best is None or n > best[0] or (n == best[0] and len(seg) < len(best[1])):
                best = (n, seg)
    return best[1] if best else []


def count(seg):
    c = dict(mfma=0, lds_read=0, lds_write=0, vmem=0, wait_lgkm=0, wait_lgkm0=0, lgkm0_between_mfma=0, wait_near_read=0, barriers=0)
    issued, seen_mfma_since_barrier, pending0 = [], False, 0        # issued: (instruction index, is a read) of the LDS operations, in order
    for at, x in enumerate(seg):
        op = x.split()[0]
        if op.startswith("v_mfma"):
            c["mfma"] += 1
            c["lgkm0_between_mfma"] += pending0
            pending0, seen_mfma_since_barrier = 0, True
        elif op.startswith("ds_read"):
            c["lds_read"] += 1
            issued.append((at, True))
        elif op.startswith("ds_write"):
            c["lds_write"] += 1
            issued.append((at, False))
        elif op.startswith(("global_load", "buffer_load")):
            c["vmem"] += 1
        elif op == "s_barrier":
            c["barriers"] += 1
            pending0, seen_mfma_since_barrier = 0, False
        elif op == "s_waitcnt" and "lgkmcnt" in x:
            c["wait_lgkm"] += 1
            if "lgkmcnt(0)" in x:
                c["wait_lgkm0"] += 1
                if seen_mfma_since_barrier:
                    pending0 += 1
            n = int(re.search(r"lgkmcnt\((\d+)\)", x).group(1))     # LDS returns in order: the wait is for the (n + 1)-th youngest operation
            if len(issued) > n and issued[-1 - n][1] and at - issued[-1 - n][0] <= 3:
                c["wait_near_read"] += 1
    return c


def taps(seg):
    run = []
    for x in seg:
        op = x.split()[0]
        if op.startswith("v_mfma"):
            print("   ", " ".join(run) if run else "-")
            run = []
        elif op.startswith("ds_"):
            run.append(op)
        elif op == "s_waitcnt":
            run.append(x.replace("s_waitcnt ", "wait:").replace(" ", ""))
        elif op == "s_barrier":
            run.append("BARRIER")
        elif op.startswith(("global_load", "buffer_load")):
            run.append("vmem")


if __name__ == "__main__":
    lines = open(sys.argv[1]).readlines()
    only = [a for a in sys.argv[2:] if a.startswith("<")]
    for name, body in functions(lines):
        t = template_args(name)
        if only and t not in only:
            continue
        md, seg = meta(lines, name), main_loop(body)
        c = count(seg)
        print(f"{t}: vgpr {md['next_free_vgpr']} sgpr {md['next_free_sgpr']} scratch {md['private_segment_fixed_size']} "
              f"lds {md['group_segment_fixed_size']} | loop: " + " ".join(f"{k} {v}" for k, v in c.items()))
        if "--taps" in sys.argv:
            taps(seg)
