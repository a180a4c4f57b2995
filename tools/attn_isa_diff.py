#!/usr/bin/env python3
"""Compare the gfx950 ISA of the NON-causal attention_kernel instantiations between two builds of attention.hip.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -save-temps -c emote_hack_amd/csrc/attention.hip   (once per tree, own directory)
    python tools/attn_isa_diff.py BEFORE/attention-hip-amdgcn-amd-amdhsa-gfx950.s AFTER/attention-hip-amdgcn-amd-amdhsa-gfx950.s

The causal flag is the kernel template's last parameter: attention_kernel<..., RES> of the old tree is attention_kernel<..., RES, false>
of the new one (mangled `...Lb<RES>EEv` -> `...Lb<RES>ELb0EEv`), and its by-value argument type is AttKernelParams (emo_attention_params
without the trailing `causal` word).  Each function body (label to .Lfunc_end) is compared with the kernel's own name masked out, the
assembler comments and the per-file basic-block label numbers dropped; exit status 1 on any difference or a kernel missing on either side."""
import re
import sys

_FN = re.compile(r"^(_Z16attention_kernel\w+):", re.M)


def bodies(path):
    text = open(path).read()
    out = {}
    for m in _FN.finditer(text):
        name = m.group(1)
        end = text.index(".Lfunc_end", m.end())
        body = re.sub(r"\s*;.*$", "", text[m.end():end].replace(name, "<kernel>"), flags=re.M)   # comments: IR block names, counters
        out[name] = re.sub(r"\.LBB\d+_", ".LBB_", body)                                            # block labels are numbered per file
    return out


def main(before, after):
    b, a = bodies(before), bodies(after)
    mapped = {re.sub(r"(Lb[01]E)(Ev)", r"\1Lb0E\2", k, count=1).replace("20emo_attention_params", "15AttKernelParams"): v for k, v in b.items()}
    bad = 0
    for name, body in sorted(mapped.items()):
        if name not in a:
            print("MISSING after:", name)
            bad += 1
        elif a[name] != body:
            print("DIFFERS:", name)
            bad += 1
    causal = [k for k in a if re.search(r"Lb[01]ELb1EEv", k)]
    print(f"{len(mapped)} non-causal instantiations compared, {bad} differ or are missing; {len(causal)} causal instantiations added")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:3]))
