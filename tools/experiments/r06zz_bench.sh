cd $GRAFT_REPO_ROOT
mkdir -p out
python bench.py --full > out/r06zz_bench.json 2> out/r06zz_bench.err
python bench.py --full --model waveflow > out/r06zz_wf_bench.json 2> out/r06zz_wf_bench.err
python bench.py --full --model wsrglow > out/r06zz_wsr_bench.json 2> out/r06zz_wsr_bench.err
for t in r06zz r06zz_wf r06zz_wsr; do python tools/profile_summary.py --shapes $t out/${t}_bench.json; cp profiles/${t}_shape_rooflines.csv out/; done
python - <<P
import json
for t in ('r06zz','r06zz_wf','r06zz_wsr'):
    d=json.loads(open('out/%s_bench.json'%t).read().strip().splitlines()[-1]); r=d['roofline']
    print(t, round(d['ms_per_step'],2), round(d['value']), 'box', round(d['box']['tflops_issued']), 'frac', round(r['frac'],4), 'fob', round(r.get('frac_of_box',0),3), 'launch_ms', round(r['launch_ms'],4), r.get('gate_conv_alone',{}).get('launch_ms'), r.get('gate_conv_alone',{}).get('frac'))
P
