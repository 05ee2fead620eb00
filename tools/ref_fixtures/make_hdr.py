#!/usr/bin/env python3
"""Execute the REFERENCE'S OWN openDR_transform (lib/OpenDRT.py:221-485) in its HDR configurations under the Taichi stand-in of
tools/ref_fixtures/standin/ and write what it computes to tests/golden/ref_opendrt_hdr.npz  (DESIGN.md §17).

    python tools/ref_fixtures/make_hdr.py

The reference runs the transform in one configuration only because of three module constants (lib/OpenDRT.py:40-44: display_gamut = Rec709,
EOTF = lin, Lp = 100).  A @ti.func body reads module constants when it runs, so setting them on the imported module and calling the function runs
the reference's text in another configuration: nothing of it is copied, only numbers leave this script (provenance and what the stand-in defines:
make.py's docstring; math = numpy float32).

Inputs: the 256 colours of the `opendrt` leaf, read from the committed tests/golden/ref_leaves.npz (its opendrt_in, which make.py:435 drew) and four rows
of their own: black, 0.18 grey, 1e4 white and (1e3, 0, 0).  Configurations (Lp, display gamut, inverse EOTF): (100, Rec709, lin) — the live one,
which ties this file to ref_leaves.npz —, (1000, Rec2020, pq), (1000, P3D65, hlg), (600, Rec709, pq), (4000, Rec2020, lin).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make  # noqa: E402  (enter_reference, GOLDEN; make.py itself is not changed)

# (peak_nits, gamut, transfer) in the numbering of include/digital_earth_hdr_output.h: gamut 0 / 1 / 2 = Rec709 / P3D65 / Rec2020 (OpenDRT's own
# numbers), transfer 0 / 1 / 2 = linear / PQ / HLG (OpenDRT's lin / pq / hlg = 0 / 4 / 5)
CONFIGS = [(100.0, 0, 0), (1000.0, 2, 1), (1000.0, 1, 2), (600.0, 0, 1), (4000.0, 2, 0)]
EXTRA = [(0.0, 0.0, 0.0), (0.18, 0.18, 0.18), (1e4, 1e4, 1e4), (1e3, 0.0, 0.0)]


def leaf_colours():
    """The `opendrt` leaf's inputs and outputs as the committed ref_leaves.npz holds them (make.py:435 drew the inputs; nothing is redrawn here)."""
    z = np.load(os.path.join(make.GOLDEN, "ref_leaves.npz"))
    return z["opendrt_in"].astype(np.float32), z["opendrt_out"].astype(np.float32)


def main():
    golden = make.GOLDEN                              # before enter_reference changes the working directory
    rgb, leaf_out = leaf_colours()
    x = np.concatenate([rgb, np.array(EXTRA, dtype=np.float32)]).astype(np.float32)
    make.enter_reference("numpy", (256, 128))
    import lib.OpenDRT as drt
    gamuts = [drt.Rec709, drt.P3D65, drt.Rec2020]
    transfers = [drt.lin, drt.pq, drt.hlg]
    outs = []
    for lp, g, t in CONFIGS:
        drt.Lp = float(lp); drt.display_gamut = gamuts[g]; drt.EOTF = transfers[t]
        with np.errstate(all="ignore"):
            rows = [list(drt.openDR_transform(float(r[0]), float(r[1]), float(r[2]))) for r in x]
        outs.append(np.asarray(rows, dtype=np.float32))
        bad = ~np.isfinite(outs[-1]).all(axis=1)
        print("Lp %6.0f gamut %d transfer %d: %d rows, %d not finite, 1e4 white -> %s" % (lp, g, t, len(rows), int(bad.sum()), outs[-1][258]), flush=True)
    drt.Lp = 100.0; drt.display_gamut = drt.Rec709; drt.EOTF = drt.lin
    same = np.array_equal(outs[0][:256], leaf_out)
    print("live configuration equals ref_leaves.npz's opendrt_out bit for bit:", same)
    np.savez_compressed(os.path.join(golden, "ref_opendrt_hdr.npz"), rgb=x, out=np.stack(outs).astype(np.float32),
                        configs=np.array(CONFIGS, dtype=np.float64),
                        note=np.array("openDR_transform of the reference executed under tools/ref_fixtures/standin (math = numpy float32) with Lp, "
                                      "display_gamut and EOTF set per row of `configs` = (peak_nits, gamut 0/1/2 = Rec709/P3D65/Rec2020, "
                                      "transfer 0/1/2 = lin/pq/hlg); rgb (260, 3) inputs, out (5, 260, 3)"))


if __name__ == "__main__":
    main()
