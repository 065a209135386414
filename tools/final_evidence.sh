# round-end evidence on the GPU box: python bench.py --full (N = 1), the same command under rocprofv3 --kernel-trace --stats, counter passes
# for the two DP kernels, smoke(), the reference's nvBowtie at speed and its kernel statistics.  Usage: tools/final_evidence.sh OUTDIR; writes
# under OUTDIR; copy what is judged into profiles/rNN/.
set -x
R=$(cd "$(dirname "$0")/.." && pwd)
O=$(mkdir -p "${1:?usage: tools/final_evidence.sh OUTDIR}" && cd "$1" && pwd)
T=$(mktemp -d)
cd "$R"
python bench.py --full --legs-file "$O/bench_legs.json" > "$O/bench_n1.json.log" 2> "$O/bench_n1.err"
cd "$T" && export TMPDIR="$T"
rocprofv3 --kernel-trace --stats --output-format csv -d "$T/pb" -o b -- python "$R/bench.py" --full --legs-file "$T/bench_prof_legs.json" > "$O/bench_prof.log" 2>&1
cp "$T"/pb/*kernel_stats.csv "$O/bench_kernel_stats.csv"
rocprofv3 --pmc SQ_INSTS_VALU SQ_WAVES --output-format csv -d "$T/pf" -o f -- python "$R/bench.py" --only full --no-cpu > "$O/pmc_full.log" 2>&1
python "$R/tools/pmc_summary.py" --each "$T"/pf/*counter_collection.csv full_gotoh > "$O/pmc_full_gotoh_each.txt" 2>&1
rocprofv3 --pmc TCC_HIT_sum TCC_MISS_sum SQ_INSTS_LDS --output-format csv -d "$T/pf2" -o f -- python "$R/bench.py" --only full --no-cpu > "$O/pmc_full2.log" 2>&1
python "$R/tools/pmc_summary.py" --each "$T"/pf2/*counter_collection.csv full_gotoh > "$O/pmc_full_gotoh_l2.txt" 2>&1
rocprofv3 --pmc SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE TCC_EA0_RDREQ_sum TCC_EA0_WRREQ_sum --output-format csv -d "$T/pf3" -o f -- python "$R/bench.py" --only full --no-cpu > "$O/pmc_full3.log" 2>&1
python "$R/tools/pmc_summary.py" --each "$T"/pf3/*counter_collection.csv full_gotoh > "$O/pmc_full_gotoh_lds.txt" 2>&1
rocprofv3 --pmc SQ_INSTS_VALU TCC_EA0_RDREQ_sum TCC_EA0_WRREQ_sum --output-format csv -d "$T/pd" -o d -- python "$R/bench.py" --only dp --no-cpu > "$O/pmc_dp.log" 2>&1
python "$R/tools/pmc_summary.py" "$T"/pd/*counter_collection.csv banded_gotoh > "$O/pmc_banded.txt" 2>&1
python "$R/tools/nvbowtie_speed.py" --reads 4000000 > "$O/nvbowtie_speed4.log" 2>&1
python "$R/tools/nvbowtie_speed.py" --reads 1000000 --wrap "rocprofv3 --kernel-trace --stats --output-format csv -d $T/pn -o n --" > "$O/nvbowtie_prof1.log" 2>&1
cp "$T"/pn/*kernel_stats.csv "$O/nvbowtie_kernel_stats.csv"
cd "$R"
python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" > "$O/smoke.log" 2>&1
