"""Every kernel launch of libn3d goes through N3D_LAUNCH (csrc/n3d_common.h): it issues an armed entry signal that no carrier kernel took
as a stand-alone launch in front (include/n3d.h, "Entry signals").  A bare <<<>>> or hipLaunchKernelGGL elsewhere would bypass that."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_launch_goes_through_n3d_launch():
    csrc = os.path.join(ROOT, "nas_3d_unet_amd", "csrc")
    files = sorted(glob.glob(os.path.join(csrc, "*.hip")) + glob.glob(os.path.join(csrc, "*.h")))
    assert files
    bad, n_launch = [], 0
    for f in files:
        text = re.sub(r"//[^\n]*", "", open(f).read())      # comments may speak of them
        n_launch += text.count("N3D_LAUNCH(")
        for i, line in enumerate(text.split("\n"), 1):
            if "hipLaunchKernelGGL" in line or "hipModuleLaunchKernel" in line or "hipExtLaunch" in line:
                bad.append((os.path.basename(f), i, line.strip()[:80]))
            if "<<<" in line:
                # the two places that may: the N3D_LAUNCH definition itself, and entry_flush() launching the signal kernel it is about
                ok = (f.endswith("n3d_common.h") and "kernel_<<<" in line) or (f.endswith("n3d_core.hip") and "sync_signal_kernel<<<" in line)
                if not ok:
                    bad.append((os.path.basename(f), i, line.strip()[:80]))
    assert not bad, bad
    assert n_launch > 100
