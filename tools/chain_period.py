"""Period of the serial track chain in a rocprofv3 --kernel-trace CSV of a pipelined run: the median distance between the starts of
successive fuse launches (k_update_insert, one per frame), and the launches and mean duration of the kernels of the chain."""
import csv, statistics, sys
rows = list(csv.DictReader(open(sys.argv[1])))
fuse = sorted(int(r["Start_Timestamp"]) for r in rows if "k_update_insert" in r["Kernel_Name"])
gaps = [b - a for a, b in zip(fuse, fuse[1:])]
print("fuse launches %d; chain period (start to start): median %.2f us, lower quartile %.2f us" % (len(fuse), statistics.median(gaps) / 1e3, statistics.quantiles(gaps, n=4)[0] / 1e3))
