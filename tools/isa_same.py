#!/usr/bin/env python3
"""Did a change of the sources change the code of a kernel?  Compares two gfx950 assembly listings (hipcc -S --cuda-device-only), or two
directories of them (*.s), kernel by kernel: functions are matched by symbol wherever they stand in either side, comments are dropped
and the per-file function index in block labels (.LBB<n>_<m> -> .LBB_<m>) is taken out, since it only says where in its file a
function stands.  Per function: SAME or DIFF, the instruction lines of both sides, VGPRs / SGPRs / scratch bytes from the kernel
descriptor, and for DIFF the difference of the opcode histograms.  Functions present on one side only are listed as ONLY.

usage: python tools/isa_same.py OLD NEW [--allow-diff] [substring of the symbol]
Exit status 1 on any DIFF or ONLY unless --allow-diff.  The tool compares text; it knows nothing about particular instructions."""
import collections
import glob
import os
import re
import sys

FUNC = re.compile(r'^([A-Za-z_$][\w$.]*):[^\n]*\n(.*?)^\.Lfunc_end\d+:', re.S | re.M)
DESC = re.compile(r'^\s*\.amdhsa_kernel\s+(\S+)\n(.*?)^\s*\.end_amdhsa_kernel', re.S | re.M)
FIELDS = (('vgpr', 'next_free_vgpr'), ('sgpr', 'next_free_sgpr'), ('scratch', 'private_segment_fixed_size'))


def normalise(body):
  out = []
  for line in body.split('\n'):
    line = re.sub(r'\s*(;|//).*$', '', line).strip()
    if line:
      out.append(re.sub(r'\.LBB\d+_', '.LBB_', re.sub(r'\s+', ' ', line)))
  return out


def read(path):
  """{symbol: (normalised lines, {vgpr, sgpr, scratch})} of a listing or of every *.s under a directory."""
  files = sorted(glob.glob(os.path.join(path, '*.s'))) if os.path.isdir(path) else [path]
  if not files:
    raise SystemExit('no listing under %s' % path)
  funcs = {}
  for f in files:
    text = open(f).read()
    desc = {}
    for m in DESC.finditer(text):
      desc[m.group(1)] = {k: int(v.group(1)) if v else None
                          for k, v in ((k, re.search(r'\.amdhsa_%s\s+(\d+)' % d, m.group(2))) for k, d in FIELDS)}
    for m in FUNC.finditer(text):
      got = (normalise(m.group(2)), desc.get(m.group(1), {}))
      if funcs.setdefault(m.group(1), got) != got:  # (a static function of a header may stand in several files, with one body)
        raise SystemExit('%s: %s is defined twice, differently' % (path, m.group(1)))
  return funcs


def opcodes(lines):
  return collections.Counter(l.split(' ')[0] for l in lines if not l.endswith(':') and not l.startswith('.'))


def compare(old, new, substr=''):
  """Prints one line per function; returns the number that are not SAME."""
  bad = 0
  for sym in sorted(set(old) | set(new)):
    if substr not in sym:
      continue
    if sym not in old or sym not in new:
      print('ONLY %s  %s' % ('old' if sym in old else 'new', sym))
      bad += 1
      continue
    (a, da), (b, db) = old[sym], new[sym]
    same = a == b and da == db
    regs = ' '.join('%s %s/%s' % (k, da.get(k), db.get(k)) for k, _ in FIELDS) if da or db else 'no descriptor'
    print('%s %s  lines %d/%d  %s' % ('SAME' if same else 'DIFF', sym, len(a), len(b), regs))
    if not same:
      bad += 1
      ha, hb = opcodes(a), opcodes(b)
      delta = ['%s %+d' % (op, hb[op] - ha[op]) for op in sorted(set(ha) | set(hb)) if ha[op] != hb[op]]
      print('     opcodes (new - old): %s' % (', '.join(delta) if delta else 'equal counts, other order or operands'))
  return bad


def main(argv):
  args = [a for a in argv if a != '--allow-diff']
  if len(args) not in (2, 3):
    raise SystemExit(__doc__)
  bad = compare(read(args[0]), read(args[1]), args[2] if len(args) == 3 else '')
  print('%d not the same' % bad)
  return 1 if bad and '--allow-diff' not in argv else 0


if __name__ == '__main__':
  sys.exit(main(sys.argv[1:]))
