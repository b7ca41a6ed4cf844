"""Per-kernel register / spill / LDS summary from hipcc -Rpass-analysis=kernel-resource-usage.

    python tools/resource_usage.py csrc/file.hip [filter]
"""
import os
import sys

from benchlib import resources


def main():
    filt = sys.argv[2] if len(sys.argv) > 2 else ""
    rows = resources(os.path.abspath(sys.argv[1]))
    if isinstance(rows.get("error"), str):
        sys.exit(rows["error"])
    for name, r in rows.items():
        if filt in name:
            print(f"{name[:90]:90s} v{r.get('VGPRs')} a{r.get('AGPRs')} occ{r.get('Occupancy')} "
                  f"vspill{r.get('VGPRs Spill')} sspill{r.get('SGPRs Spill')} lds{r.get('LDS Size')}")


if __name__ == "__main__":
    main()
