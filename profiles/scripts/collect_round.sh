set -x
ROOT=$(cd "$(dirname "$0")/../.." && pwd)
O=$GRAFT_REPO_ROOT/gpurun_out/${ROUND_TAG:-r03c}; mkdir -p $O
cd $GRAFT_REPO_ROOT
python bench.py --full --parity-trained 4 > $O/bench.json 2> $O/bench.err
python bench.py --full --analysis bf16 > $O/bench_bf16.json 2>/dev/null
python bench.py --full --model joint --batch 4 > $O/bench_joint.json 2>/dev/null
python bench.py --full --model joint --batch 8 --no-cpu-baseline > $O/bench_joint_b8.json 2>/dev/null
python bench.py --full --dtype f32 --steps 20 > $O/bench_f32.json 2>/dev/null
python bench.py --full --sweep --batch 4 --steps 16 > $O/bench_c5_sweep.json 2>/dev/null
python bench.py --full --sweep --model joint --batch 4 --steps 16 > $O/bench_c5_sweep_joint.json 2>/dev/null
HESIC_FORCE_COLLECTIVES=1 python bench.py --full --mode train > $O/bench_train.json 2>/dev/null
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats -d /tmp/p1 -o d --output-format csv -- python "$ROOT/bench.py" --full --steps 5 --warmup 2 --no-cpu-baseline --exec eager > /dev/null 2>&1
cp /tmp/p1/d_kernel_stats.csv $O/default_kernel_stats.csv
HESIC_NO_OVERLAP=1 rocprofv3 --kernel-trace --stats -d /tmp/p2 -o s --output-format csv -- python "$ROOT/bench.py" --full --steps 5 --warmup 2 --no-cpu-baseline --exec eager > /dev/null 2>&1
cp /tmp/p2/s_kernel_stats.csv $O/single_stream_kernel_stats.csv
HESIC_NO_OVERLAP=1 rocprofv3 --pmc FETCH_SIZE --kernel-include-regex "igemm_glds_kernel|igemm_tr4_kernel|n2w_gdn_hilo" --output-format csv -d $O/pmc_f -- python $GRAFT_REPO_ROOT/profiles/scripts/forward_n.py hsic 4 > /dev/null 2>&1
HESIC_NO_OVERLAP=1 rocprofv3 --pmc WRITE_SIZE --kernel-include-regex "igemm_glds_kernel|igemm_tr4_kernel|n2w_gdn_hilo" --output-format csv -d $O/pmc_w -- python $GRAFT_REPO_ROOT/profiles/scripts/forward_n.py hsic 4 > /dev/null 2>&1
i=0
for set in "SQ_BUSY_CYCLES SQ_WAVE_CYCLES SQ_VALU_MFMA_BUSY_CYCLES" "SQ_ACTIVE_INST_ANY SQ_WAIT_INST_ANY SQ_WAIT_ANY" "SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_MFMA" "SQ_INSTS_LDS SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE" "SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_LDS SQ_ACTIVE_INST_VMEM"; do
  i=$((i+1))
  HESIC_NO_OVERLAP=1 timeout 300 rocprofv3 --pmc $set --kernel-include-regex "igemm_glds_kernel|igemm_tr4_kernel|n2w_gdn_hilo|sconv_n2w|sconv_w2n" --output-format csv -d $O/pmcsq/p$i -- python $GRAFT_REPO_ROOT/profiles/scripts/forward_n.py hsic 3 > /dev/null 2>&1
done
python $GRAFT_REPO_ROOT/profiles/make_pmc_sq_json.py $O/pmcsq $O/pmc_sq.json > $O/pmc_sq.txt 2>&1
rocprofv3 --kernel-trace --stats -d /tmp/p3 -o t --output-format csv -- python $GRAFT_REPO_ROOT/profiles/scripts/train_step.py --size 512 --only g --steps 10 > /dev/null 2>&1
cp /tmp/p3/t_kernel_stats.csv $O/graphed_train_step_512_kernel_stats.csv
ls -la $O $O/pmc_f/* | head -40
du -sh $O
