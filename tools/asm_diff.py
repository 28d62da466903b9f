#!/usr/bin/env python3
"""asm_diff.py OLD.s NEW.s — compare two `hipcc -S --cuda-device-only` outputs of one translation unit kernel by kernel.

Instructions are compared as text after dropping comments, directives and blank lines and renumbering basic-block labels
(.LBB<function>_<block> changes with every function added in front).  Prints one line per kernel: same / differs / only in one
file, and the instruction counts; exit status 0."""
import re
import sys


def kernels(path):
    out, name, body = {}, None, []
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            name, body = m.group(1), []
            out[name] = body
            continue
        if name is None:
            continue
        if line.startswith(".Lfunc_end"):
            name = None
            continue
        text = line.split(";")[0].strip()
        if not text or (text.startswith(".") and not text.startswith(".LBB")):
            continue
        body.append(re.sub(r"\.LBB\d+_", ".LBB_", text))
    return out


def main():
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    for name in sorted(set(old) | set(new)):
        if name not in old:
            print("only-new  %6d  %s" % (len(new[name]), name))
        elif name not in new:
            print("only-old  %6d  %s" % (len(old[name]), name))
        elif old[name] == new[name]:
            print("same      %6d  %s" % (len(new[name]), name))
        else:
            print("differs   %6d -> %6d  %s" % (len(old[name]), len(new[name]), name))


if __name__ == "__main__":
    main()
