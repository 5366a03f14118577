#!/usr/bin/env python3
"""Diff the ISA of the ordinary srbd13 solve kernels of two builds of csrc/sddp_inst.hip compiled with --save-temps:

    python profiles/resume/isa_diff.py PARENT.s BRANCH.s

(hipcc -O3 --offload-arch=gfx950 -std=c++17 -fPIC -Iinclude -Isrbd_horizon_amd/csrc -DSDDP_INST_MODEL=Srbd13 -DSDDP_INST_FN=ops_srbd13
 '-DSDDP_INST_NAME="srbd13"' --save-temps -c srbd_horizon_amd/csrc/sddp_inst.hip; the file is sddp_inst-hip-amdgcn-amd-amdhsa-gfx950.s.)
Comments are dropped and basic-block labels lose their function number; what is left is compared line by line."""
import difflib
import re
import sys

PARENT, BRANCH = sys.argv[1], sys.argv[2]
def body(path, pat):
    L=open(path).read().split('\n')
    for i,l in enumerate(L):
        if re.match(r'^_ZN4sddp'+pat+r'.*:\s*(;.*)?$', l):
            j=i
            while not L[j].startswith('.Lfunc_end'): j+=1
            return L[i+1:j]
def norm(lines):
    out=[]
    for l in lines:
        l=re.sub(r';.*$','',l).rstrip(); l=re.sub(r'\.LBB\d+_','.LBB_',l)
        if l.strip(): out.append(l)
    return out
M=r'INS_9SrbdModelILi2ELb0ELb0ELb0ELi0EvEE'
for name,pb,pp in (("solve_kernel_w2<srbd13>", '15solve_kernel_w2'+M+'Lb0EJEEE', '15solve_kernel_w2'+M+'JEEE'),
                   ("solve_kernel<srbd13>", '12solve_kernel'+M+'Lb0EJEEE', '12solve_kernel'+M+'JEEE'),
                   ("solve_kernel_w2<srbd13, table>", '15solve_kernel_w2'+M+'Lb0EJPK', '15solve_kernel_w2'+M+'JPK'),
                   ("solve_kernel<srbd13, table>", '12solve_kernel'+M+'Lb0EJPK', '12solve_kernel'+M+'JPK')):
    nb=norm(body(BRANCH,pb)); np_=norm(body(PARENT,pp))
    d=[x for x in difflib.unified_diff(np_,nb,lineterm='',n=0) if not x.startswith(('---','+++','@@'))]
    print(f"{name}: parent {len(np_)} lines, branch {len(nb)} lines, differing lines {len(d)}")
    for x in d[:6]: print('   ',x)
