#!/usr/bin/env python3
"""Writes cfpnet_amd/colormaps.py: the uint8 [256,3] colour tables `cfpnet_amd.render` looks values up in, taken once from
matplotlib so that nothing under cfpnet_amd/ imports it:

    table = matplotlib.colormaps[name](np.arange(256), bytes=True)[:, :3]

for `magma_r` (the default of the reference's `colorize`, src/utils/utils.py:44), `magma`, `viridis`, `turbo` and `jet`.  The module
holds each table as text -- 256 entries of six hexadecimal digits, rrggbb, eight to a line -- so that the tables are reviewable source
and no binary file sits in the package.  tests/test_render_abi.py pins the bytes by digest and compares them with matplotlib wherever
matplotlib is installed."""
import os

import numpy as np

NAMES = ("magma_r", "magma", "viridis", "turbo", "jet")

HEADER = '''"""The colour tables of `cfpnet_amd.render`, written by tools/gen_colormaps.py from matplotlib {version}:
`matplotlib.colormaps[name](np.arange(256), bytes=True)[:, :3]`.  Generated; do not edit.  Each table is 256 entries of six
hexadecimal digits, rrggbb, in index order."""
import numpy as np

_HEX = {{
'''

FOOTER = '''}

NAMES = tuple(_HEX)


def table(name: str) -> np.ndarray:
    """uint8 [256,3] (a new array)."""
    t = np.frombuffer(bytes.fromhex("".join(_HEX[name].split())), dtype=np.uint8).reshape(256, 3).copy()
    return t
'''


def tables():
    import matplotlib
    return {n: np.ascontiguousarray(matplotlib.colormaps[n](np.arange(256), bytes=True)[:, :3]).astype(np.uint8) for n in NAMES}


if __name__ == "__main__":
    import matplotlib
    out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cfpnet_amd", "colormaps.py")
    text = HEADER.format(version=matplotlib.__version__)
    for n, t in tables().items():
        words = ["%02x%02x%02x" % tuple(int(v) for v in row) for row in t]
        lines = [" ".join(words[i:i + 8]) for i in range(0, 256, 8)]
        text += f'    "{n}": """\n' + "\n".join(lines) + '\n""",\n'
    with open(out, "w") as f:
        f.write(text + FOOTER)
    print(f"{out}: {', '.join(NAMES)}")
