"""tools/kernel_resource_diff.py — registers / spills / scratch of every kernel, this tree against a git revision (default: the
end of round 2): which kernels changed their budget?  Per kernel: (VGPRs, SGPRs, VGPR spills, SGPR spills, scratch bytes, static LDS bytes).
(cross-compiles, no GPU; found the chain-kernel occupancy regression of round 3)"""
import re, subprocess, os, sys, tempfile
ROOT=os.path.dirname(os.path.dirname(os.path.abspath(__file__))); T=os.path.join(tempfile.gettempdir(),'waa_resource_diff')
os.makedirs(T, exist_ok=True)
FLAGS=["--offload-arch=gfx950","-O3","-std=c++17","-fPIC","-ffp-contract=off","-fgpu-flush-denormals-to-zero","--cuda-device-only","-S"]
def res(path, inc):
    out=T+'/'+os.path.basename(path)+'.s'   # (never next to the sources: make has a built-in rule  %: %.s)
    r=subprocess.run([os.environ.get('HIPCC','/opt/rocm/bin/hipcc')]+FLAGS+['-I'+inc,'-I'+ROOT+'/include',path,'-o',out],stderr=subprocess.PIPE)
    if r.returncode: return None
    text=open(out).read(); d={}
    for m in re.finditer(r"\.group_segment_fixed_size:\s+(\d+)(.*?)\.wavefront_size", text, re.S):   # (one kernel's metadata, keys in order)
        b=m.group(2); g=lambda k:int(re.search(r"\.%s:\s+(\d+)"%k,b).group(1))
        d[re.search(r"\.name:\s+(\S+)",b).group(1)]=(g('vgpr_count'),g('sgpr_count'),g('vgpr_spill_count'),g('sgpr_spill_count'),g('private_segment_fixed_size'),int(m.group(1)))
    return d
old=sys.argv[1] if len(sys.argv) > 1 else '236a9b1'
inc_old=T+'/inc_old'; os.makedirs(inc_old,exist_ok=True)
files=subprocess.check_output(['git','-C',ROOT,'ls-tree','--name-only',old,'web-audio-api-rs_amd/csrc/']).decode().split()
for f in files:
    if f.endswith(('.hpp','.hip')):   # (.hip too: waa_iir_inst.hip includes waa_iir_stream.hip)
        open(inc_old+'/'+os.path.basename(f),'wb').write(subprocess.check_output(['git','-C',ROOT,'show',old+':'+f]))
same=changed=0; only_new=[]
for f in files:
    if not f.endswith('.hip'): continue
    b=os.path.basename(f)
    po=T+'/old_'+b; open(po,'wb').write(subprocess.check_output(['git','-C',ROOT,'show',old+':'+f]))
    ro=res(po,inc_old); rn=res(ROOT+'/'+f, ROOT+'/web-audio-api-rs_amd/csrc')
    if ro is None or rn is None: print(b,'compile problem'); continue
    for k in sorted(set(ro)&set(rn)):
        if ro[k]!=rn[k]: print(b, k[:90], 'old',ro[k],'new',rn[k]); changed+=1
        else: same+=1
    only_new+=[(b,k) for k in sorted(set(rn)-set(ro))]
    for k in sorted(set(rn)-set(ro)): print(b, k[:90], 'new kernel', rn[k])
for f in sorted(os.listdir(ROOT+'/web-audio-api-rs_amd/csrc')):
    if f.endswith('.hip') and 'web-audio-api-rs_amd/csrc/'+f not in files:
        rn=res(ROOT+'/web-audio-api-rs_amd/csrc/'+f, ROOT+'/web-audio-api-rs_amd/csrc')
        only_new+=[(f,k) for k in sorted(rn or {})]
        for k in sorted(rn or {}): print(f, k[:90], 'new file', rn[k])
print('%d kernels compared with %s: %d unchanged, %d changed; %d kernels only in this tree'%(same+changed, old, same, changed, len(only_new)))
