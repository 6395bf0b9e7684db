"""Where one kernel's loops wait for their loads, from a hipcc -S dump (tuning aid; a reader of the listing for people).
usage: python tools/isa_waits.py k.s <mangled-kernel-name-substring> [min loop length, default 150]

A loop is the span of text from a label to the last branch back to it; loads of a loop that starts inside it are shown with
that loop only.  For every global or flat load of a loop it prints the first s_waitcnt that waits for it, with the number of
instructions between the two.  vmcnt counts loads and stores in the order of issue, so vmcnt(N) waits for a load only once N
or more memory instructions were issued behind it: "behind" is the count at the wait that is listed, and an earlier wait with
a larger N is passed over.  Where the loop's text ends first, the search goes on at the loop's head ("next iter").

All of this is in the order of the text.  Both sides of a branch inside the loop count, so a distance is an upper bound of
what one pass executes, a wait on the other side of a branch from the load can be listed as the load's, and memory
instructions of a side not taken can make a wait look as if it covered the load: read the listing where it matters."""
import re
import sys

path, key = sys.argv[1], sys.argv[2]
min_len = int(sys.argv[3]) if len(sys.argv) > 3 else 150
lines = open(path).read().split("\n")
start = next(i for i, l in enumerate(lines) if l.startswith("_Z") and key in l and ":" in l)
end = next(i for i in range(start, len(lines)) if lines[i].strip().startswith("s_endpgm"))

# the kernel's instructions, each with the label of its block
insts, labels, block = [], {}, "entry"
for l in lines[start + 1:end + 1]:
    s = l.split(";")[0].strip()
    m = re.match(r"^(\.LBB\d+_\d+):", s)
    if m:
        block = m.group(1)
        labels[block] = len(insts)
        continue
    if not s or s.startswith("."):
        continue
    insts.append((block, s))

loops = {}
for i, (b, s) in enumerate(insts):
    op = s.split()[0]
    if op.startswith("s_cbranch") or op.startswith("s_branch"):
        head = labels.get(s.split()[-1])
        if head is not None and head <= i:
            loops[head] = max(loops.get(head, 0), i)
loops = sorted(loops.items())


def is_load(s):
    return s.startswith("global_load") or s.startswith("flat_load") or s.startswith("buffer_load")


def is_vmem(s):      # what vmcnt counts on gfx9: vector memory loads, stores and atomics
    return s.startswith(("global_", "flat_", "buffer_", "scratch_"))


def vm_wait(s):
    m = re.match(r"s_waitcnt.*vmcnt\((\d+)\)", s)
    return int(m.group(1)) if m else None


print("%s: %d instructions, %d loops" % (lines[start].split(":")[0], len(insts), len(loops)))
for head, tail in loops:
    inner = [(h, t) for h, t in loops if head < h <= tail]      # (a loop that starts inside: block placement may move its tail out)
    own = [i for i in range(head, tail + 1) if is_load(insts[i][1]) and not any(h <= i <= t for h, t in inner)]
    if tail - head + 1 < min_len or not own:
        continue
    n_flat = sum(insts[i][1].startswith("flat_load") for i in own)
    print("\nloop %s .. %s: %d instructions, %d loads of its own (%d flat)" % (insts[head][0], insts[tail][0], tail - head + 1, len(own), n_flat))
    # LDS instructions of the loop's text by kind (both sides of a branch count), and its full drains of the LDS queue
    kinds = {}
    for i in range(head, tail + 1):
        op = insts[i][1].split()[0]
        if op.startswith("ds_"):
            kinds[op] = kinds.get(op, 0) + 1
    drains = sum(1 for i in range(head, tail + 1) if re.match(r"s_waitcnt.*lgkmcnt\(0\)", insts[i][1]))
    print("  LDS: %s; s_waitcnt lgkmcnt(0): %d" % (", ".join("%s %d" % kv for kv in sorted(kinds.items())) or "none", drains))
    for i in own:
        order = list(range(i + 1, tail + 1)) + list(range(head, i))
        behind, hit = 0, None
        for j in order:
            n = vm_wait(insts[j][1])
            if n is not None and n <= behind:
                hit = j
                break
            behind += is_vmem(insts[j][1])
        what = " ".join(insts[i][1].replace(",", " ").split()[:2])
        if hit is None:
            print("  %-10s +%-4d %-34s no wait for it in the loop" % (insts[i][0], i - head, what))
            continue
        print("  %-10s +%-4d %-34s -> %-10s +%-4d %-30s %2d behind %4d between%s" % (
            insts[i][0], i - head, what, insts[hit][0], hit - head, insts[hit][1], behind, order.index(hit), "  (next iter)" if hit < i else ""))
