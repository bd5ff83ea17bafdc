"""CPU estimate of the march's jump over empty ground (DESIGN.md §5 Skip 5), made before it was
built: with the oracle's first hits of 8 of the 256 C2 poses (every 2nd descending ring, every
4th azimuth), walk each ray's in-box samples up to its first hit, once probing every sample and
once letting a ray jump by the horizontal clearance of the cell and level it probes (a Euclidean
distance transform of "a point at or below the level's top" on 0.06 m cells, less 1.5 cells).
Prints the probes of both walks, the first hits a jump passed over (must be 0) and per-ring
counts.  Needs the oracle (make -C oracle), numpy and scipy.
usage: python tools/fan_clearance_estimate.py > profiles/fan_clearance_estimate.log"""
import sys, math, numpy as np
sys.path.insert(0,'.'); sys.path.insert(0,'oracle')
from pointcloud_processor_amd import synth
import pyoracle
from scipy import ndimage
sc = synth.terrain_scene()
T = sc.terrain[:, :3].astype(np.float64)
r=0.056; R=r+0.001
p=sc.area[:, :3].astype(np.float64); res=0.1
bbox=np.array([p[:,0].min()-res,p[:,0].max()+res,p[:,1].min()-res,p[:,1].max()+res,p[:,2].min()-res,p[:,2].max()+res])
Tc=pyoracle.Cloud(sc.terrain)
poses=pyoracle.generate_candidates(Tc,bbox,pyoracle.vl_params(num_candidates=348),sc.zx120_pose5)[:256]
print("poses",poses.shape, "xy range", poses[:,0].min(),poses[:,0].max(),poses[:,1].min(),poses[:,1].max(), "yaw uniq",np.unique(poses[:,4]).size)
sel=poses[::32]
n_az,n_el=1024,256
elmin,elmax=-85*np.pi/180,85*np.pi/180
blocked,units,fh=pyoracle.raycast_fan(Tc,sel,n_az,n_el,elmin,elmax,15.0,True)
print("blocked",blocked,"units",units)
ca,sa,ce,se=pyoracle.fan_tables(n_az,n_el,elmin,elmax)
S=[0.5]
while S[-1]+0.3<15-0.08: S.append(S[-1]+0.3)
S=np.array(S); K=len(S); print("K",K)
lo=T.min(0)-R; hi=T.max(0)+R
cf=0.06; c=0.12
ox,oy,oz=lo[0],lo[1],lo[2]
fnx=int((hi[0]-ox)/cf)+2; fny=int((hi[1]-oy)/cf)+2
ix=((T[:,0]-ox)/cf).astype(int); iy=((T[:,1]-oy)/cf).astype(int)
zmin=np.full((fny,fnx),np.inf); np.minimum.at(zmin,(iy,ix),T[:,2])
zmin_d=ndimage.minimum_filter(zmin,size=3,mode='constant',cval=np.inf)
nl=int((hi[2]-oz)/c)+1
D=[]
for L in range(nl):
    ztop=oz+(L+1)*c
    M=zmin_d<=ztop+R
    d=ndimage.distance_transform_edt(~M)  # cells to nearest True
    D.append(np.maximum(d-1.5,0)*cf)
D=np.stack(D)
print("levels",nl,"grid",fny,fnx)
tot_base=tot_skip=0; viol=0; nrays=0; nhit=0
ring_base=np.zeros(n_el); ring_skip=np.zeros(n_el)
azs=np.arange(0,n_az,4)
for pi,P in enumerate(sel):
    px,py,pz,pitch,yaw=P
    cy,sy=math.cos(yaw),math.sin(yaw)
    for j in range(0,n_el,2):
        lx=ce[j]*ca[azs]; ly=ce[j]*sa[azs]
        dx=cy*lx-sy*ly; dy=sy*lx+cy*ly; dz=se[j]
        if dz>=0: continue
        f=fh[pi,j,azs].astype(int)
        endk=np.where(f>=0,f,K-1)
        nxt=np.zeros(len(azs),int)
        hs=0.3*ce[j]
        for k in range(K):
            s=S[k]
            qx=px+dx*s; qy=py+dy*s; qz=pz+dz*s
            inb=(qx>lo[0])&(qx<hi[0])&(qy>lo[1])&(qy<hi[1])&(qz>lo[2])&(qz<hi[2])
            a0=inb&(k<=endk)
            b=a0.sum(); tot_base+=b; ring_base[j]+=b
            a1=a0&(k>=nxt)
            viol+=(a0&(f==k)&(k<nxt)).sum()
            b1=a1.sum(); tot_skip+=b1; ring_skip[j]+=b1
            if b1:
                fx=np.clip(((qx-ox)/cf).astype(int),0,fnx-1); fy=np.clip(((qy-oy)/cf).astype(int),0,fny-1)
                L=min(max(int((qz-oz)/c),0),nl-1)
                d=D[L][fy,fx]
                n=np.floor(d/max(hs,1e-9)).astype(int)
                n=np.minimum(n,1000)
                nxt=np.where(a1,k+1+n,nxt)
        nrays+=len(azs); nhit+=(f>=0).sum()
print("rays",nrays,"hit",nhit,"probes base",tot_base,"with skip",tot_skip,"ratio",tot_skip/tot_base,"violations",viol)
print("per-ray probes base",tot_base/nrays,"skip",tot_skip/nrays)
for j in range(0,124,6): print(j, int(ring_base[j]), int(ring_skip[j]))
