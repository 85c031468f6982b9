"""Count the Jacobi sweeps of dh3d_gnc_rigid's fits on the fixtures of tools/registration_bench.py (64 pairs x 512 at 50 %,
20 % and 0 % inliers, the same generator and seed), on the CPU: a numpy port of csrc/rigid_fit.h rotation_from_b's sweep
loop applied to every B the restatement (tests/gnc_reference.py) forms.  The sweep count is the one data-dependent cost
inside a fit; a call ends with its slowest workgroup, so the largest per-pair total is what the time follows.

    python tools/gnc_sweeps.py
"""
import os
import sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np, gnc_reference as g, registration_reference as ref
def rows(rng,P,M,D,share):
    x=(rng.random((P,M,3))*40-20).astype(np.float32); y=x+np.float32(3.0)
    da=rng.standard_normal((P,M,D)).astype(np.float32)
    out=rng.random((P,M))>=share
    y[out]=(rng.random((int(out.sum()),3))*40-20).astype(np.float32)
    return x,y
def sweeps(Bm):
    a=Bm.copy(); n=0
    for sweep in range(32):
        off=sum(a[r][c]*a[r][c] for r in range(4) for c in range(r+1,4))
        if not off>0: break
        n+=1
        for p in range(3):
            for q in range(p+1,4):
                apq=a[p][q]
                if abs(apq)<=1e-18*(abs(a[p][p])+abs(a[q][q])):
                    a[p][q]=a[q][p]=0.0; continue
                th=(a[q][q]-a[p][p])/(2*apq)
                t=(1.0 if th>=0 else -1.0)/(abs(th)+np.sqrt(th*th+1))
                c=1/np.sqrt(t*t+1); s=t*c; tau=s/(1+c)
                a[p][p]-=t*apq; a[q][q]+=t*apq; a[p][q]=a[q][p]=0.0
                for k in range(4):
                    if k!=p and k!=q:
                        gg,h=a[k][p],a[k][q]
                        a[k][p]=a[p][k]=gg-s*(h+gg*tau); a[k][q]=a[q][k]=h+s*(gg-h*tau)
    return n
count=[0]
orig=ref._b_matrix
def hook(X,Y):
    B=orig(X,Y); count[0]+=sweeps(B[0]); return B
ref._b_matrix=hook
rng=np.random.default_rng(0)
rows(rng,64,512,128,0.5)
for share in (0.5,0.2,0.0):
    x,y=rows(rng,64,512,128,share)
    tot=[];its=[]
    for p in range(64):
        count[0]=0
        r=g.gnc(x[p],y[p])
        tot.append(count[0]); its.append(r['iterations'])
    tot=np.array(tot); its=np.array(its)
    print(share,'fits',its.min(),its.max(),'sweeps per pair: mean %.1f min %d max %d; per fit mean %.2f'%(tot.mean(),tot.min(),tot.max(),(tot/its).mean()))
