"""Per-event kernel breakdown of `scripts/brush_batch_latency.py --trace` under `rocprofv3 --kernel-trace --output-format csv`.
The script separates its warm-up from the timed events by an idle gap of about a second; this takes the dispatches after the
largest gap in the trace, divides by the number of timed events and prints one JSON line: per kernel the launches and the
device time per event, the sum of kernel time per event, and the event's wall span on the device (first start to last end).
usage: python scripts/summarize_brush_batch_trace.py <..._kernel_trace.csv> <timed events>"""
import csv
import json
import sys
from collections import defaultdict


def main(path, events):
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    starts = [int(r["Start_Timestamp"]) for r in rows]
    gap_at = max(range(1, len(rows)), key=lambda i: starts[i] - int(rows[i - 1]["End_Timestamp"]))
    timed = rows[gap_at:]
    per = defaultdict(lambda: [0, 0])
    for r in timed:
        name = r["Kernel_Name"].split("(")[0].replace("void ", "")
        per[name][0] += 1
        per[name][1] += int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
    kern = sorted(({"kernel": k, "launches_per_event": round(v[0] / events, 2), "us_per_event": round(v[1] / events / 1e3, 2)}
                   for k, v in per.items()), key=lambda d: -d["us_per_event"])
    span = (int(timed[-1]["End_Timestamp"]) - int(timed[0]["Start_Timestamp"])) / events / 1e3
    print(json.dumps({"events": events, "launches_per_event": round(len(timed) / events, 1),
                      "kernel_us_per_event": round(sum(d["us_per_event"] for d in kern), 1),
                      "device_span_us_per_event": round(span, 1), "kernels": kern}))


if __name__ == "__main__":
    main(sys.argv[1], int(sys.argv[2]))
