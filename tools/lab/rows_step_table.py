"""Per-kernel table of the last N replayed batched decode steps in a rocprofv3 kernel trace (a step starts at decode_step_begin_rows_kernel).
usage: python tools/lab/rows_step_table.py <kernel_trace.csv> [N = 24]"""
import csv, collections, sys, re
rows=list(csv.DictReader(open(sys.argv[1])))
rows.sort(key=lambda r:int(r["Start_Timestamp"]))
begins=[i for i,r in enumerate(rows) if "decode_step_begin_rows_kernel" in r["Kernel_Name"]]
N=int(sys.argv[2]) if len(sys.argv) > 2 else 24
i0=begins[-N]
sel=rows[i0:]
steps=[]
b=[i-i0 for i in begins[-N:]]+[len(sel)]
per=[len(sel[b[k]:b[k+1]]) for k in range(N)]
assert len(set(per))==1, per
span=[(int(sel[b[k+1]-1]["End_Timestamp"])-int(sel[b[k]]["Start_Timestamp"]))/1e6 for k in range(N)]
tot=sum(int(r["End_Timestamp"])-int(r["Start_Timestamp"]) for r in sel)/1e3/N
agg=collections.OrderedDict()
for r in sel:
    name=r["Kernel_Name"]
    short=re.sub(r"\(.*$","",name) if "<" not in name else name.split("(")[0]
    key=(name, f'({r["Grid_Size_X"]},{r["Grid_Size_Y"]},{r["Grid_Size_Z"]})', r["LDS_Block_Size"])
    d=agg.setdefault(key,[0,0.0]); d[0]+=1; d[1]+=(int(r["End_Timestamp"])-int(r["Start_Timestamp"]))/1e3
print(f"# dispatches per step: {per[0]}; first dispatch to last dispatch per step = {sum(span)/N:.3f} ms; sum of kernel times per step = {tot/1e3:.3f} ms")
print("kernel | grid (x,y,z) | LDS bytes | dispatches per step | us per dispatch | us per step | share")
for (n,g,l),(c,t) in sorted(agg.items(), key=lambda kv:-kv[1][1]):
    print(f"{n[:110]} | {g} | {l} | {c//N} | {t/c:.1f} | {t/N:.1f} | {t/N/tot:.3f}")
