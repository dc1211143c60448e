#!/usr/bin/env python3
"""Per-kernel resource and instruction-mix table of one csrc/*.hip file (developer tool; needs hipcc, no GPU).

    python tools/isa_report.py dlpm_amd/csrc/conv_wino4.hip [--keep-asm PATH]

Compiles the file device-only to gfx950 assembly with the flags of dlpm_amd/build.py (DLPM_BUILD_DEFS / DLPM_BUILD_FLAGS apply) plus
-Rpass-analysis=kernel-resource-usage, and prints per kernel: VGPRs, AGPRs, SGPRs, scratch bytes per lane, occupancy (waves per SIMD),
LDS bytes, and how many instructions of each class its body holds -- v_mfma*, ds_read* / ds_write*, global_load* / global_store*,
buffer_*, scratch_*, s_barrier, s_waitcnt.  Two runs (two commits, two sets of defines) are compared with diff: the table is sorted
by kernel name and holds nothing that changes from run to run."""
import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from dlpm_amd.build import FLAGS, HIPCC

CLASSES = [('mfma', r'v_mfma'), ('ds_rd', r'ds_read|ds_load'), ('ds_wr', r'ds_write|ds_store'), ('g_ld', r'global_load'),
           ('g_st', r'global_store'), ('buffer', r'buffer_'), ('scratch', r'scratch_'), ('barrier', r's_barrier'), ('waitcnt', r's_waitcnt')]
REMARKS = [('vgpr', 'VGPRs'), ('agpr', 'AGPRs'), ('sgpr', 'TotalSGPRs'), ('scr', 'ScratchSize [bytes/lane]'), ('occ', 'Occupancy [waves/SIMD]'),
           ('lds', 'LDS Size [bytes/block]')]


def compile_asm(src, asm):
    cmd = [HIPCC] + FLAGS + ['-x', 'hip', '--cuda-device-only', '-S', '-Rpass-analysis=kernel-resource-usage', src, '-o', asm]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        sys.exit('hipcc failed:\n%s\n%s' % (' '.join(cmd), r.stderr))
    return r.stderr


def parse_remarks(text):
    """{mangled name: {field: int}} from the kernel-resource-usage remarks"""
    res, cur = {}, None
    for line in text.splitlines():
        m = re.search(r'remark: .*Function Name: (\S+)', line)
        if m:
            cur = res.setdefault(m.group(1), {})
            continue
        if cur is None or 'remark:' not in line:
            continue
        for key, label in REMARKS:
            m = re.search(r'remark:\s+' + re.escape(label) + r': (\d+)', line)
            if m:
                cur[key] = int(m.group(1))
    return res


def parse_asm(path, names):
    """{mangled name: {class: count}}: the instructions between a kernel's label and its .Lfunc_end"""
    res, cur = {}, None
    pats = [(k, re.compile(r'\s+(?:%s)' % p)) for k, p in CLASSES]
    with open(path) as f:
        for line in f:
            if cur is None:
                m = re.match(r'(\w+):', line)
                if m and m.group(1) in names:
                    cur = res.setdefault(m.group(1), dict.fromkeys([k for k, _ in CLASSES], 0))
                continue
            if line.startswith('.Lfunc_end'):
                cur = None
                continue
            for k, pat in pats:
                if pat.match(line):
                    cur[k] += 1
                    break
    return res


def demangle(names):
    filt = shutil.which('llvm-cxxfilt') or shutil.which('c++filt')
    if not filt:
        return dict(zip(names, names))
    out = subprocess.run([filt] + names, capture_output=True, text=True).stdout.split('\n')
    short = {}
    for n, d in zip(names, out):
        d = re.sub(r'\(anonymous namespace\)::|dlpm::', '', d)
        short[n] = re.sub(r'^void\s+|\(.*$', '', d)    # kernel<template arguments>, parameter list dropped
    return short


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('source', help='a .hip file of dlpm_amd/csrc')
    ap.add_argument('--keep-asm', metavar='PATH', help='leave the assembly there')
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        asm = args.keep_asm or os.path.join(tmp, 'out.s')
        usage = parse_remarks(compile_asm(args.source, asm))
        counts = parse_asm(asm, set(usage))
    names = demangle(sorted(usage))
    cols = [k for k, _ in REMARKS] + [k for k, _ in CLASSES]
    print('# %s   flags: %s' % (os.path.basename(args.source), ' '.join(FLAGS)))
    print('%-44s' % 'kernel' + ''.join('%8s' % c for c in cols))
    for n in sorted(usage, key=lambda n: names[n]):
        row = dict(usage[n], **counts.get(n, {}))
        print('%-44s' % names[n] + ''.join('%8s' % row.get(c, '-') for c in cols))


if __name__ == '__main__':
    main()
