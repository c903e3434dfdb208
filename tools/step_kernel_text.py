# python3 tools/step_kernel_text.py FILE.s: the text of every gemm_step_kernel<MODE, TGT> of a device assembly file (hipcc ... --offload-device-only -S), the instantiations in
# name order, without the assembler's comments and without the function's ordinal in its local labels (.LBB16_4 -> .LBB_4: it changes when other kernels are merged)
import re, sys
fn, out = None, {}
for line in open(sys.argv[1]):
    m = re.match(r'(_ZN2mi4gemm16gemm_step_kernelILi\d+ELi\d+EEEvNS0_10StepParamsE):', line)
    if m: fn = m.group(1); out[fn] = []
    elif re.match(r'\.Lfunc_end\d+:', line): fn = None
    if fn:
        t = re.sub(r'BB\d+_', 'BB_', re.sub(r'\s*;.*', '', line.rstrip()))
        if t: out[fn].append(t)
for k in sorted(out): print('\n'.join(out[k]))
