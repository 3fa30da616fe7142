#!/bin/bash
# Build container (no GPU needed): compile the library for gfx950 with the given extra flags and print, per kernel,
# registers, spills, occupancy, LDS, code size (codeLenInByte) and instruction counts by class from the ISA listing.
#   tools/isa_stats.sh [-DFLAG ...]      (listing left in /tmp/isa/mi355rast-hip-amdgcn-amd-amdhsa-gfx950.s)
ROOT=$(cd "$(dirname "$0")/.." && pwd)
mkdir -p /tmp/isa && cd /tmp/isa || exit 1
/opt/rocm/bin/hipcc -O3 --offload-arch=gfx950 -ffp-contract=off -fPIC -shared -std=c++17 --save-temps "$@" \
    -o /tmp/isa/lib.so "$ROOT/py-numpy-renderer_amd/csrc/mi355rast.hip" 2>/dev/null || { echo "compile failed"; exit 1; }
python3 - <<'PY'
import re
s = open('/tmp/isa/mi355rast-hip-amdgcn-amd-amdhsa-gfx950.s').read()
# a kernel: its label, its body up to .Lfunc_end, then the "; Kernel info:" comment block
for m in re.finditer(r'^(_ZN2mr\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:\n(.*?)COMPUTE_PGM_RSRC2:USER_SGPR', s, re.S | re.M):
    name, body, info = m.group(1), m.group(2), m.group(3)
    if '.amdhsa_kernel' not in body and 'Kernel info' not in info:
        continue
    short = re.sub(r'^_ZN2mr\d+', '', name)[:28]
    def g(key):
        r = re.search(r'; %s *[:=] *(\d+)' % key, info)
        return int(r.group(1)) if r else -1
    # bytes in front of the MR_HOT_END marker: 4 per instruction, 8 where it carries a 32-bit literal or is a 64-bit encoding
    # (VOP3 / SMEM / DS / FLAT / MUBUF ...: everything but SOP*, VOP1 / VOP2 / VOPC in their short form), estimated from the text
    def size(l):
        op = l.split()[0]
        wide = op.endswith(('_e64', '_dpp', '_sdwa')) or op.split('_')[0] in ('global', 'buffer', 'flat', 'scratch', 'ds') or \
            op.startswith(('s_load', 's_buffer_load', 's_memtime', 's_memrealtime', 'v_fma', 'v_mad', 'v_add_f64', 'v_mul_f64', 'v_readlane', 'v_writelane', 'v_lshl_add', 'v_cndmask_b32_e64', 'v_pk_', 'v_mfma'))
        lit = bool(re.search(r'(0x[0-9a-f]{3,}|\b\d{3,}\b)', l.split(';')[0].split(None, 1)[1] if len(l.split(None, 1)) > 1 else ''))
        return 8 if (wide or lit) else 4
    code_lines = [l for l in body.split('\n') if l.startswith('\t') and not l.startswith('\t.')]
    hot = next((i for i, l in enumerate(code_lines) if 'MR_HOT_END' in l), None)
    hot_bytes = sum(size(l) for l in code_lines[:hot] if not l.startswith('\t;')) if hot is not None else -1
    ins = [l.split()[0] for l in body.split('\n') if l.startswith('\t') and not l.startswith('\t.') and not l.startswith('\t;')]
    valu = sum(1 for i in ins if i.startswith('v_'))
    salu = sum(1 for i in ins if i.startswith('s_') and not i.startswith(('s_load', 's_buffer_load', 's_waitcnt', 's_nop', 's_cbranch', 's_branch', 's_setpc', 's_barrier')))
    br = sum(1 for i in ins if i.startswith(('s_cbranch', 's_branch', 's_setpc')))
    wait = sum(1 for i in ins if i.startswith(('s_waitcnt', 's_nop')))
    f64 = sum(1 for i in ins if i.startswith('v_') and 'f64' in i)
    rl = sum(1 for i in ins if i.startswith('v_readlane') or i.startswith('v_writelane'))
    sm = sum(1 for i in ins if i.startswith('s_load') or i.startswith('s_buffer_load'))
    vm = sum(1 for i in ins if i.split('_')[0] in ('global', 'buffer', 'flat', 'scratch'))
    ds = sum(1 for i in ins if i.startswith('ds_'))
    print(f"{short:28s} vgpr {g('NumVgprs'):3d} sgpr {g('TotalNumSgprs'):3d} scratch {g('ScratchSize'):3d} occ {g('Occupancy'):2d} "
          f"lds {g('LDSByteSize'):6d} code {g('codeLenInByte'):6d} B hot ~{hot_bytes:6d} B | instr {len(ins):5d} valu {valu:5d} salu {salu:5d} branch {br:4d} wait {wait:4d} f64 {f64:4d} rd/wrlane {rl:4d} smem {sm:3d} vmem {vm:3d} ds {ds:3d}")
PY
