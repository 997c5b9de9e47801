/*
 * csim.h -- C-ABI of the MI355X batched MNA solve engine (libcsim.so).
 *
 * extern "C", plain pointers and sizes, no C++/torch types, no exceptions
 * across the boundary: every call returns 0 (CSIM_OK) or a negative error and
 * csim_last_error() describes it.  Per-instance trouble (non-convergence,
 * non-finite solve, tiny pivot) never fails a call: it is reported in the
 * per-instance status words (CSIM_ST_* in csim_ir.h), so one bad instance
 * cannot kill a batch -- this replaces the reference's stderr WARNINGs and
 * its std::runtime_error (src/tanalisis.cpp:360-376, src/dcanalysis.cpp:135-158).
 *
 * There is NO CPU backend behind this ABI.  csim_engine_create() fails with
 * CSIM_ERR_NO_DEVICE when no HIP device is usable; nothing falls back to host
 * arithmetic.  (The CPU restatement lives in oracle/ and is test-only.)
 *
 * Reference interface each group replaces (ZyuRao/CircuitSimulator):
 *   csim_netlist_*        parseNetlist()                 include/parser.hpp:67-75
 *                         Circuit::assignEquationIndices src/circuit.cpp:42-61  (src/main.cpp:29,34)
 *   csim_dc_batch*        computeDcOperatingPoint()      include/tanalisis.hpp:9
 *                         dcSolve/dcSolveLU              include/dcanalysis.hpp:8-14, src/dcanalysis.cpp:242-262
 *   csim_tran_batch*      runTransientAnalysisBackwardEuler  include/tanalisis.hpp:15-17, src/tanalisis.cpp:83-424
 *   csim_lu_solve_batch   Solver::solveLinearSystemLU / luDecompose  include/solver.hpp:30-131
 *   (stamping)            Element::stamp virtuals        include/element.hpp:28-31, src/element.cpp:9-307
 *                         -- no entry point of their own: the stamps run inside the DC/TRAN kernels.
 *
 * Data layout.  Every per-instance table is "slot-major": element [i][b] at
 * i*B + b, b = instance.  That is the coalesced layout for the
 * lane-per-instance kernels and costs the wave-per-instance kernels one
 * strided read per launch.  The *_dev entry points take DEVICE pointers in
 * that layout and enqueue on the given HIP stream; the host-pointer entry
 * points take the instance-major tables proposed in SURVEY.md 8(b) ([B][P],
 * [B][N]) and do the copies and transposes.
 *
 * Arithmetic.  The general kernels, the "faithful" generated kernels (transient and DC) and the kernels for
 * linear circuits perform the reference's floating-point operations in the reference's order (the device's
 * sin() may differ from glibc's in the last bit).  The FAST generated transient kernels (family "scheduled":
 * one, four and sixteen lanes per instance) deviate deliberately, inside the 1e-9 bar, NR counts equal: FMA
 * contraction; one refined reciprocal per pivot instead of a division per multiplier; four-/sixteen-lane kernels:
 * matrix assembled as (step-constant part) + (MOSFET part), back substitution in descending column order, the
 * recorded pivot accepted where a LATER row exceeds it by less than 8 ulp (the reference would swap: the two
 * pivots then agree to 15 digits; include/solver.hpp:48-56), the update norm summed across lanes; convergence
 * decided on the squared norm.  A convergence decision within 2e-8 (relative) of its threshold is re-done by
 * the faithful kernel and rolled back if it falls the other way; steps that do not contract at the damping
 * rate, and factorisations no recorded pivot sequence fits, are handed to the faithful / general kernels.
 * What remains: a step whose update norm lands within ~1e-9 of the tolerance is decided by the last bits of the
 * whole trajectory; measured on dbmixer.sp, a fast family takes one NR pass more or less than the faithful
 * family about once per 1e10 step decisions.  csim_engine_set_kernel(eng, 3) selects the
 * faithful family outright.
 *
 * Streams.  With the default option hybrid_sync = 1 a *_dev call that runs
 * generated ("scheduled") kernels WAITS on its stream once per stage of the
 * hand-over ladder to read two flag words -- usually once per call -- and
 * returns as soon as no instance is left unfinished.  With hybrid_sync = 0
 * such a call only enqueues (a fixed sequence of launches, each returning at
 * once when it finds nothing to do) and never waits: use that to overlap
 * streams (copies or collectives of one launch's results under the next launch).
 * Graph capture is NOT supported (step_first is a kernel argument, and a replayed
 * capture did not reproduce a direct call reliably: tools/dev/graph_capture_probe.py).
 * Calls on engines without a generated
 * kernel never wait.  An engine owns ONE set of hand-over buffers: calls on
 * the same engine must be ordered with respect to each other (same stream, or
 * event-ordered); use one engine per concurrent stream.
 */
#ifndef CSIM_H
#define CSIM_H

#include <stdint.h>
#include "csim_ir.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CSIM_OK                0
#define CSIM_ERR_ARG          -1   /* null pointer, bad size                       */
#define CSIM_ERR_IO           -2   /* netlist file cannot be opened                */
#define CSIM_ERR_NO_DEVICE    -3   /* no usable HIP device: there is no CPU path   */
#define CSIM_ERR_HIP          -4   /* a HIP runtime call failed                    */
#define CSIM_ERR_UNSUPPORTED  -5   /* circuit outside what the kernels cover       */
#define CSIM_ERR_EMPTY        -6   /* circuit has no unknowns                      */
#define CSIM_ERR_CONFIG       -7   /* invalid .TRAN / .AC / .NOISE / .DISTO / .STB / .PZ numbers, no AC source, no port, no probe */

typedef struct csim_netlist csim_netlist;
typedef struct csim_engine  csim_engine;

const char* csim_last_error(void);
const char* csim_version(void);

/* ---------------------------------------------------------------- netlist
 * Parse + index a netlist (host only, runs once, microseconds).             */
int  csim_netlist_parse_file(const char* path, csim_netlist** out);
/* same, from memory (what a rank receives from the broadcast of the netlist) */
int  csim_netlist_parse_text(const char* text, int64_t len, csim_netlist** out);
void csim_netlist_free(csim_netlist* nl);

/* flattened circuit; owned by the netlist, valid until csim_netlist_free */
const csim_ir* csim_netlist_ir(const csim_netlist* nl);
/* "Circuit summary" numbers of src/main.cpp:36-41 */
int  csim_netlist_counts(const csim_netlist* nl, int32_t* n_nodes, int32_t* n_elems,
                         int32_t* n_unknowns, int32_t* n_node_eq, int32_t* n_branch_eq);
/* nominal parameter vector, P doubles */
int  csim_netlist_nominal_params(const csim_netlist* nl, double* out);
/* node name (node equations) or element name (branch equations) of equation eq */
const char* csim_netlist_eq_name(const csim_netlist* nl, int32_t eq);
/* equation index of a node name, -1 for ground, -2 if unknown */
int  csim_netlist_node_eq(const csim_netlist* nl, const char* node_name);
/* .TRAN card (src/parser.cpp:497-524) */
int  csim_netlist_tran(const csim_netlist* nl, int32_t* enabled, double* tstep, double* tstop, double* tstart);
/* node-voltage probes named by .PLOTNV / .PRINT cards, as equation indices */
int  csim_netlist_num_probes(const csim_netlist* nl);
int  csim_netlist_probe_eq(const csim_netlist* nl, int32_t i);
/* .DC cards (src/parser.cpp:476-495): source element index and sweep numbers */
int  csim_netlist_num_dc_sweeps(const csim_netlist* nl);
int  csim_netlist_dc_sweep(const csim_netlist* nl, int32_t i, int32_t* src_elem,
                           double* start, double* stop, double* step);
/* .DC sweep as a batch axis (the reference parses the card and never executes it,
 * src/parser.cpp:476-495; src/main.cpp never reads sim.dcSweeps): sweep point j is the
 * nominal circuit with the swept source's dcValue replaced by start + j*step.
 * points = floor((stop-start)/step + 1e-9) + 1, 0 for step == 0, a step of the wrong sign
 * or a card whose source is not a V/I element.                                        */
int64_t csim_netlist_dc_sweep_points(const csim_netlist* nl, int32_t i);
/* parameter table [P][n_points] (slot-major) + the swept values [n_points]              */
int  csim_netlist_dc_sweep_params(const csim_netlist* nl, int32_t i, int64_t n_points,
                                  double* params, double* values);
/* header line of the reference's transient CSV (src/tanalisis.cpp:191-206):
 * "time,V(<node>)...,I(<elem>)..."; returns the length needed (excl. NUL) */
int  csim_netlist_csv_header(const csim_netlist* nl, char* buf, int32_t cap);
/* .AC card (src/parser.cpp:526-549): sweep 0 DEC, 1 OCT, 2 LIN                   */
int  csim_netlist_ac(const csim_netlist* nl, int32_t* enabled, int32_t* sweep, int32_t* n_points,
                     double* fstart, double* fstop);
/* AC excitation of element `elem` (`AC mag [phase_deg]` on a V/I line; 0, 0 for any other element).
 * Kept beside the IR, not in the parameter vector: P and the slots are those of the netlist without AC. */
int  csim_netlist_ac_source(const csim_netlist* nl, int32_t elem, double* mag, double* phase_deg);
/* .NOISE V(out[,ref]) [src] DEC|OCT|LIN n fstart fstop: output equations (out_m_eq -1: ground; -2: a node the
 * netlist does not have), input source element (-1: none named, or no such element), the sweep as for .AC.      */
int  csim_netlist_noise(const csim_netlist* nl, int32_t* enabled, int32_t* out_p_eq, int32_t* out_m_eq,
                        int32_t* src_elem, int32_t* sweep, int32_t* n_points, double* fstart, double* fstop);
/* Noise generators ("Noise analysis" below), in element order: element index and the two equations the current
 * generator lies between (-1: ground).  Resistors between their terminals, MOSFET channels drain - source.    */
int  csim_netlist_num_noise_sources(const csim_netlist* nl);
int  csim_netlist_noise_source(const csim_netlist* nl, int32_t i, int32_t* elem, int32_t* eq_a, int32_t* eq_b);
/* Ports of "S-parameter analysis" below: V sources carrying `PORTNUM k [Z0 r]`, in port order (port k is index k - 1).
 * The values are kept beside the IR like the AC excitation: P, the slots and the Monte-Carlo draws are those of the
 * netlist without the tokens.  csim_netlist_num_ports: the number of ports (0 .. 4), or CSIM_ERR_CONFIG when the
 * numbering has a gap or a duplicate, or there are more than 4 ports.                                              */
int  csim_netlist_num_ports(const csim_netlist* nl);
int  csim_netlist_port(const csim_netlist* nl, int32_t i, int32_t* elem, int32_t* branch_eq, double* z0);
/* .SP DEC|OCT|LIN n fstart fstop: the sweep as for .AC */
int  csim_netlist_sp(const csim_netlist* nl, int32_t* enabled, int32_t* sweep, int32_t* n_points, double* fstart,
                     double* fstop);
/* .SP ... 1: the card's trailing donoise token ("Two-port noise analysis" below); 0 without a card, without the
 * token, or with any other sixth token.                                                                         */
int  csim_netlist_sp_noise(const csim_netlist* nl, int32_t* donoise);
/* Monte-Carlo recipe per parameter slot: 0 fixed, 1 scaled by (1+sigma z),
 * 2 MOS K rebuilt from a MU draw: K = (MU(1+sigma z))*COX*(W/L)              */
int  csim_netlist_mc_kinds(const csim_netlist* nl, int32_t* kinds);

/* ----------------------------------------------------------------- engine */
/* One engine per (circuit, device).  Uploads the circuit plan; owns only its
 * handle and device scratch.  CSIM_ERR_NO_DEVICE if `device` is not a usable
 * HIP device.                                                                */
int  csim_engine_create(const csim_netlist* nl, int32_t device, csim_engine** out);
void csim_engine_destroy(csim_engine* eng);
/* which transient kernel the engine will use: "general" (wave-per-instance,
 * dense LDS LU with dynamic pivoting), "scheduled" (circuit-specialised code with
 * a verified pivot schedule) or "faithful" (the same with the reference's arithmetic) */
const char* csim_engine_tran_kernel(const csim_engine* eng);
/* description of the loaded generated library ("" if none): circuit, pivot schedules, LDS doubles
 * per lane, and the floating-point operations ONE solve on the first schedule executes
 * ("ops_per_solve: fma=.. mul=.. addsub=.. recip=.. cmp=..")                                   */
const char* csim_engine_sched_info(const csim_engine* eng);
/* lanes per instance the scheduled transient kernel would use for a batch of B instances (1, 4 or 16;
 * 0 = the general kernel runs: one 64-lane wavefront per instance).  A linear circuit's library has one
 * transient kernel: 16 (tape and iterate in registers) or 1 (larger circuits), whatever B is.        */
int  csim_engine_lanes_for_batch(const csim_engine* eng, int32_t B);
/* force a kernel family: 0 = auto, 1 = general only, 2 = scheduled required, 3 = the generated kernel
 * with the reference's arithmetic ("faithful": true divisions, no FMA contraction, steps at the NR cap
 * kept and flagged; bit-faithful on recorded pivot sequences, run-time pivoting kernel for the rest)    */
int  csim_engine_set_kernel(csim_engine* eng, int32_t which);

/* Run-time options of one engine, as text.  The environment variable named with each key is read
 * ONCE, in csim_engine_create, as the key's default; nothing on a hot path reads the environment.
 *   hybrid_rounds (CSIM_HYBRID_ROUNDS, 4)   hand-back rounds between the scheduled and the general
 *                                           kernel per transient call
 *   hybrid_steps  (CSIM_HYBRID_STEPS, 64)   most steps the general kernel keeps an instance per round
 *   lanes_per_instance (CSIM_LANES_PER_INSTANCE, 0)  scheduled transient kernel: 1 = lane per instance,
 *                                           4 = four lanes per instance (circuits of up to 32 unknowns),
 *                                           16 = sixteen lanes per instance (up to 96 unknowns), 0 = chosen by batch size
 *                                           (<= 4096: 16; up to 16 384: 4; beyond: 1)
 *   sched_variant (CSIM_SCHED_VARIANT, 0)   tuning kernels of a generated library (2 rich, 10+k sweep)
 *   auto_jit (CSIM_AUTO_JIT, off)           csim_tran_batch specialises a new circuit on first use
 *   jit_dir (CSIM_JIT_DIR; default $XDG_CACHE_HOME/csim_jit or /tmp/csim_jit.<uid>)  JIT cache: created
 *                                           0700; must be a real directory of the calling user, not
 *                                           writable by group/others; only regular files of the calling
 *                                           user are ever loaded from it
 *   hipcc (CSIM_HIPCC, /opt/rocm/bin/hipcc), jit_timeout (CSIM_JIT_TIMEOUT, 600 s)
 *   jit_dc_alts (CSIM_JIT_DC_ALTS, 4), jit_dc_force (CSIM_JIT_DC_FORCE, off)  DC schedules kept by the JIT
 *   jit_gen_opts                            generator options of this engine's JIT, "key=value,key=value"
 *                                           (near_band, near_band_dc, stage_ahead, group4, place_search, ...:
 *                                           engine/codegen.hpp), set on top of the options the shipped libraries
 *                                           are generated with (GeneratorOptions::engineDefaults);
 *                                           they are part of the hash a cached library is checked against
 *   near_test_rollback (0)                  test aid: every verified near-threshold decision is treated as a
 *                                           mismatch, so the roll-back path runs (results must not change)
 *   hybrid_sync (CSIM_HYBRID_SYNC, 1)       see "Streams" above
 *   ac_kernel (auto)                        AC, noise, S-parameter, distortion and loop-gain sweep kernel, auto | wave | packed (test aid) | block
 *                                           (opt-in: AC and noise of up to 1024 unknowns; see csim_ac_batch_dev)
 *   dc_fast (CSIM_DC_FAST, 0)               DC operating points start on the fast generated kernel (FMA
 *                                           contraction, reciprocal pivots; controller decisions within
 *                                           its rounding noise are replayed) instead of the faithful one
 *   pss_tol (2e-6), pss_max_rounds (20), pss_chunk (0)  periodic steady state, see csim_pss_batch_dev
 * Unknown key or bad value: CSIM_ERR_ARG.                                                        */
int  csim_engine_set_option(csim_engine* eng, const char* key, const char* value);
/* Counters of one engine since its creation (-1: unknown key).  Maintained in synchronous mode
 * (hybrid_sync = 1) only:
 *   "near_verified"      near-threshold convergence decisions of the fast transient kernels that the
 *                        faithful kernel re-did (src/tanalisis.cpp:369; DESIGN.md "near-threshold guard")
 *   "near_rolled_back"   of those, the ones whose pass count differed: the instance was rolled back
 * A constant of the engine, in any mode:
 *   "ac_chunk"           the largest number of instances the small-signal sweeps (AC, noise, S-parameter)
 *                        assemble and solve at once; a larger batch runs in chunks of this size           */
int64_t csim_engine_stat(const csim_engine* eng, const char* key);

/* Monte-Carlo parameter table on the device: instance b_first+i of the global
 * batch -> column i.  Instance 0 is the nominal circuit.  Counter-based:
 * any shard regenerates any instance from (seed, instance, slot).            */
int  csim_mc_params_dev(csim_engine* eng, uint64_t seed, double sigma, int64_t b_first,
                        int32_t B, double* d_params /*[P][B]*/, void* stream);
/* host mirror of the same generator (bit-identical; for fixtures and tests)  */
int  csim_mc_params_host(const csim_netlist* nl, uint64_t seed, double sigma, int64_t b_first,
                         int32_t B, double* params /*[P][B]*/);

/* DC operating point of B instances.                                         */
int  csim_dc_batch_dev(csim_engine* eng, const double* d_params /*[P][B]*/, int32_t B,
                       double* d_x /*[N][B]*/, int32_t* d_iters /*[B]*/,
                       uint32_t* d_status /*[B]*/, void* stream);

/* n_steps backward-Euler time steps for B instances, steps
 * step_first+1 .. step_first+n_steps of the run (t = step*tstep).
 *   d_x      in: state at step_first (the DC solution for step_first == 0);
 *            out: state after the last step.  Histories (capacitor voltages,
 *            inductor currents, MOS junction voltages) are functions of the
 *            previous state, so x is the whole per-instance state.
 *   d_wave   optional [n_rows_total][n_probe][B]: row r holds step r*out_stride
 *            (row 0 = t=0 state, written when step_first == 0).
 *   d_iters  [B], accumulated (+=): NR iterations.   d_status [B], OR-ed.
 *   d_step_iters optional [n_steps][B] NR iterations of each step of this call */
int  csim_tran_batch_dev(csim_engine* eng, const double* d_params /*[P][B]*/, int32_t B,
                         double tstep, int64_t step_first, int64_t n_steps,
                         const int32_t* probe_eq /*host*/, int32_t n_probe, int32_t out_stride,
                         double* d_wave, double* d_x /*[N][B]*/, int64_t* d_iters,
                         uint32_t* d_status, int32_t* d_step_iters, void* stream);

/* Host-pointer forms.  params [B][P] instance-major (NULL =
 * nominal for every instance), x_out/x_final [B][N].                          */
int  csim_dc_batch(csim_engine* eng, const double* params, int32_t B,
                   double* x_out, int32_t* nr_iters, uint32_t* status);
/* Runs DC then the whole transient.  wave_out optional
 * [B][n_rows][n_probe], n_rows = floor(nSteps/out_stride)+1 minus rows with
 * t < tstart (suppressed like dumpRow, src/tanalisis.cpp:208-209).  Waveforms
 * are streamed out in chunks while the next chunk is computed; device memory
 * does not grow with the length of the run.  CSIM_AUTO_JIT=1 in the
 * environment specialises a circuit without a prebuilt kernel on first use.   */
int  csim_tran_batch(csim_engine* eng, const double* params, int32_t B,
                     double tstep, double tstop, double tstart,
                     const int32_t* probe_eq, int32_t n_probe, int32_t out_stride,
                     double* wave_out, double* x_final, int64_t* nr_iters, uint32_t* status);
/* The transient of ONE instance of a batch description, written as the reference's CSV
 * (src/tanalisis.cpp:189-231: header "time,V(<node>)...,I(<source or inductor>)...", values "%.9e", one row per
 * time step, rows with t < tstart suppressed) -- what plot_tran.py reads.  For the Monte-Carlo instances one
 * wants to look at; the whole batch's waveforms go through csim_tran_batch's wave_out.
 *   params    [B][P] instance-major host table or NULL (nominal); `instance` picks its row
 *   probe_eq  columns (equation indices) in file order; n_probe == 0: the netlist's .PLOTNV / .PRINT probes
 *             when it names any (src/parser.cpp:630-723), else every unknown -- the reference's own file
 * Runs the DC operating point and the transient of that instance alone (a batch of one on the engine's
 * kernels) and formats on the host.  CSIM_ERR_IO if the file cannot be written.                       */
int  csim_tran_write_csv(csim_engine* eng, const double* params, int32_t B, int32_t instance,
                         double tstep, double tstop, double tstart,
                         const int32_t* probe_eq, int32_t n_probe, const char* path);
/* number of rows csim_tran_batch writes per instance for these numbers       */
int64_t csim_tran_num_rows(double tstep, double tstop, double tstart, int32_t out_stride);
int64_t csim_tran_num_steps(double tstep, double tstop);

/* ---- AC small-signal analysis (.AC; the reference parses the card and never runs it) ----
 * The small-signal limit of this engine's own backward-Euler transient (csim_tran_batch), linearised at a DC
 * operating point x_op:  (G + j w C) v = J,  w = 2 pi f (pi = csim_consts.pi).
 *   G  the transient matrix with every companion term removed: resistors 1/R, V-source and inductor incidence
 *      (+-1), the MOSFET Jacobian gd, gg, gs of mos_eval at x_op (src/element.cpp:181-274; cst unused),
 *      tran_gmin on every node row (src/tanalisis.cpp:356).
 *   C  capacitors C; MOSFET Cgs = Cgd = Cj0/2, Csb = Cdb = Cj0 (src/tanalisis.cpp:334-352); an inductor adds -L on
 *      its branch diagonal (branch row Vp - Vm - j w L I = 0).  An element the transient leaves out is left out
 *      here too, incidence included: C <= 0, L <= 0, Cj0 <= 0.
 *   J  the AC excitations only, mag (cos phi, sin phi), phi = deg pi / 180, stamped as stampAC does
 *      (src/element.cpp:68-81,125-151); DC values and waveforms do not enter.
 * Assembled once per instance with the transient's gather order, then for every frequency a complex LU with
 * partial pivoting in the shape of Solver::solveLinearSystemLU: pivot = the first row with the largest
 * re^2 + im^2 (strict '>'); a maximum below lu_eps^2 gives the zero vector for that (instance, frequency) and
 * sets CSIM_ST_LU_TINY_PIVOT in the instance's status; the rest of the sweep goes on.  Multiplier
 * a conj(p) (1 / |p|^2), back substitution in ascending column order, no FMA contraction.  Circuits of up to
 * 63 unknowns, of up to 1024 with the engine option ac_kernel=block (CSIM_ERR_UNSUPPORTED beyond); no source with
 * mag != 0: CSIM_ERR_CONFIG.
 *
 * Frequency grid (SPICE): DEC fstart 10^(k/n), OCT fstart 2^(k/n), k = 0 .. floor(n log_b(fstop/fstart) + 1e-9);
 * LIN n points from fstart to fstop inclusive (n == 1: fstart).  n <= 0, fstart <= 0 (DEC/OCT) or fstop < fstart:
 * CSIM_ERR_CONFIG.                                                                                              */
int64_t csim_ac_num_freqs(int32_t sweep, int32_t n_points, double fstart, double fstop);   /* < 0: error */
int  csim_ac_freqs(int32_t sweep, int32_t n_points, double fstart, double fstop, double* f);
/* Enqueues the sweep; never waits for it.  A new frequency or probe list is uploaded once (a synchronous copy into
 * a buffer that no sweep still enqueued reads, so calls may follow each other on a stream without a
 * synchronisation in between), then cached.
 *   d_xop    [N][B] operating points (csim_dc_batch_dev)     freqs   host [F], Hz
 *   probe_eq host, NULL = every unknown (n_probe ignored)    d_out   [F][n_probe][B] complex (re, im) pairs
 *   d_status [B], OR-ed
 * The engine option ac_kernel (test aid) forces the sweep kernel: "wave" (one wavefront per system, N <= 63) or
 * "packed" (registers, 32 lanes per system, N <= 32); "auto" picks packed for N <= 32.  Both give bit-identical
 * results.
 * ac_kernel=block is opt-in and never picked by "auto": one 256-thread workgroup per system with the matrix in a
 * device scratch, 1 <= N <= 1024, for AC and noise analysis (csim_ac_*, csim_noise_*); the same arithmetic in the
 * same order, so bit-identical to the other two where they run.  With it the S-parameter and two-port noise entry
 * points return CSIM_ERR_UNSUPPORTED, and csim_engine_stat("ac_chunk") counts its scratch.                      */
int  csim_ac_batch_dev(csim_engine* eng, const double* d_params /*[P][B]*/, int32_t B, const double* d_xop,
                       const double* freqs, int32_t F, const int32_t* probe_eq, int32_t n_probe,
                       double* d_out, uint32_t* d_status, void* stream);
/* DC operating point, then the sweep.  params [B][P] or NULL (nominal); freqs NULL = the netlist's .AC card
 * (F ignored); out [B][F][n_probe] complex; status [B]: DC and AC bits.                                      */
int  csim_ac_batch(csim_engine* eng, const double* params, int32_t B, const double* freqs, int32_t F,
                   const int32_t* probe_eq, int32_t n_probe, double* out, uint32_t* status);
/* The linearised system itself, per instance (enqueue only): d_sys [B][2N^2 + 2N] = G column-major [N][N],
 * C column-major [N][N], J re [N], J im [N].                                                                    */
int  csim_ac_system_dev(csim_engine* eng, const double* d_params /*[P][B]*/, int32_t B, const double* d_xop,
                        double* d_sys, void* stream);

/* ---- Noise analysis (.NOISE; small-signal output noise by one adjoint solve per frequency) ----
 * For instance b and angular frequency w let A = G + j w C be exactly the matrix of "AC analysis" above (the same
 * assembly: an element AC leaves out is left out here).
 *   Adjoint system  A^T y = d, d real: +1 at equation out_p, -1 at out_m (out_m = -1: ground, no entry).
 *      out_p == out_m or out_p < 0: CSIM_ERR_ARG.  The solve is the AC algorithm applied to the matrix A^T: the same
 *      pivot rule on the transposed matrix, multiplier, elimination order, zero-multiplier skip and ascending back
 *      substitution.  Load A^T(i,j) = G(j,i) + j (w C(j,i)), w C one product.  No FMA contraction anywhere.
 *   Generators  in element order, S per circuit (csim_netlist_noise_source), each a current PSD in A^2/Hz between two
 *      equations (a, b).  kT4 = 4.0 * 1.380649e-23 * temp_k, computed once on the host.
 *        resistor, R != 0:  psd = kT4 * (1.0 / R)      (R == 0: psd 0, the stamp is skipped, src/element.cpp:20-24)
 *        MOSFET channel, drain - source (SPICE3 MOS1):  psd = kT4 * ((2.0 / 3.0) * fabs(gg)), gg the gate
 *        transconductance of mos_eval at x_op, the call the G pass makes.
 *      Noiseless: capacitors, inductors, sources, tran_gmin, the MOS off-conductance.  No flicker noise (the model
 *      cards carry no KF / AF).
 *   Per generator s   z = y[a] - y[b] (ground = (0, 0));  contrib[s] = (z.re z.re + z.im z.im) * psd[s]
 *   Output noise      onoise = 0.0 + contrib[0] + contrib[1] + ... in ascending order, V^2/Hz
 *   Gain (src_elem >= 0)  H = transfer from a unit AC excitation of that V / I element to the output, read off the
 *      adjoint: V source with branch equation k: H = y[k]; I source (p, m): H = y[m] - y[p] (stampAC,
 *      src/element.cpp:68-81).  Any other element: CSIM_ERR_ARG.  Input-referred noise is onoise / |H|^2, formed by
 *      the caller.
 *   Failed factorisation  a column maximum below lu_eps^2 at some frequency: onoise, every contrib and the gain are
 *      +0.0 there, CSIM_ST_LU_TINY_PIVOT is OR-ed into the instance's status, the sweep goes on.
 * Circuits of up to 63 unknowns, 1024 with ac_kernel=block (CSIM_ERR_UNSUPPORTED beyond).  S == 0 is legal: onoise = 0.  temp_k <= 0 or not
 * finite: CSIM_ERR_CONFIG.  No AC source is needed.
 *
 * Enqueues the sweep; never waits for it; frequency lists as csim_ac_batch_dev (same buffers, same discipline).
 *   d_onoise [F][B]    d_gain [F][B] complex (re, im) or NULL (not written when src_elem < 0)
 *   d_contrib [F][S][B] or NULL    d_psd [S][B] or NULL: the generators' PSDs    d_status [B], OR-ed
 * The engine option ac_kernel picks the kernel as for AC; both give bit-identical results.                        */
int  csim_noise_batch_dev(csim_engine* eng, const double* d_params /*[P][B]*/, int32_t B, const double* d_xop,
                          const double* freqs, int32_t F, int32_t out_p_eq, int32_t out_m_eq, int32_t src_elem,
                          double temp_k, double* d_onoise, double* d_gain, double* d_contrib, double* d_psd,
                          uint32_t* d_status, void* stream);
/* DC operating point, then the sweep.  params [B][P] or NULL (nominal); freqs NULL = the grid of the netlist's
 * .NOISE card (F ignored); out_p_eq == -2 = the card's output and source (out_m_eq, src_elem ignored); no card:
 * CSIM_ERR_CONFIG.  onoise [B][F]; gain [B][F] complex or NULL; contrib [B][F][S] or NULL; psd [B][S] or NULL.   */
int  csim_noise_batch(csim_engine* eng, const double* params, int32_t B, const double* freqs, int32_t F,
                      int32_t out_p_eq, int32_t out_m_eq, int32_t src_elem, double temp_k, double* onoise,
                      double* gain, double* contrib, double* psd, uint32_t* status);

/* ---- S-parameter analysis (.SP; Y and S of the declared ports by one factorisation per frequency) ----
 * Ports.  A V source becomes port k by `PORTNUM k [Z0 r]` after its DC / waveform / AC tokens (ngspice's spelling,
 *   any case).  k runs 1 .. P without a gap or a duplicate, P <= 4; Z0 defaults to 50 and must be finite and > 0.
 *   PORTNUM on anything but a V source is a parse error (reported, the statement dropped, like the other card
 *   errors).  Card: `.SP DEC|OCT|LIN n fstart fstop`, the grid of csim_ac_freqs.
 * System.  For instance b and angular frequency w, A = G + j w C is exactly the matrix of "AC analysis" above: the
 *   same assembly, the same elements left out, tran_gmin.  For port j the right-hand side is the real unit vector at
 *   the branch equation k_j of its V source.  Every `AC mag` of the netlist is ignored; all other V sources are AC
 *   shorts and I sources open, which is what a zero right-hand side says.
 * Multi-RHS solve.  The AC algorithm carried to K right-hand-side columns n .. n+K-1 of the augmented matrix: pivot
 *   search, exchange, multiplier and zero-multiplier skip unchanged; the elimination runs j = k+1 .. n+K-1; the back
 *   substitution runs per column.  Pivoting never looks at a right-hand side, so column c of the result is bit for
 *   bit the single-RHS solve with that column alone.  A column maximum below lu_eps^2 makes all K vectors +0.0 and
 *   sets CSIM_ST_LU_TINY_PIVOT.
 * Y(i,j) = -x(j)[k_i], both parts negated: the branch current of the V-source stamp flows from the + node through
 *   the source to the - node, the current into the network at + is its negative.  A resistor R across a single port
 *   gives Y = +1/R.
 * S.  s_i = sqrt(Z0_i), computed once on the host.  M(i,j) = delta_ij + (s_i * Y(i,j)) * s_j, the two products in
 *   that order on re and im separately, the diagonal as 1.0 + re.  M X = 2 I by the same multi-RHS solve with n = P,
 *   K = P and the same lu_eps.  S(i,j) = X(i,j) - delta_ij, only the real part and only on the diagonal touched:
 *   S = (I - y)(I + y)^-1 = 2 (I + y)^-1 - I with y the normalised admittance.
 * Failures.  M fails its pivot test: S of that (instance, frequency) is all +0.0, Y is kept, the flag is set.  A
 *   fails: Y and S are both +0.0.  The sweep goes on either way.
 * No FMA contraction anywhere.  Circuits of up to 63 unknowns (CSIM_ERR_UNSUPPORTED beyond); no port, or a bad port
 * numbering: CSIM_ERR_CONFIG.  No AC source is needed.
 *
 * Enqueues the sweep; never waits for it; frequency lists as csim_ac_batch_dev (same buffers, same discipline).
 *   d_y, d_s [F][P][P][B] complex (re, im), row i then column j, instance fastest; d_s may be NULL; d_status [B], OR-ed
 * The engine option ac_kernel picks the kernel as for AC; both give bit-identical results.                        */
int  csim_sp_batch_dev(csim_engine* eng, const double* d_params /*[P][B]*/, int32_t B, const double* d_xop,
                       const double* freqs, int32_t F, double* d_y, double* d_s, uint32_t* d_status, void* stream);
/* DC operating point, then the sweep.  params [B][P] or NULL (nominal); freqs NULL = the grid of the netlist's .SP
 * card (F ignored; no card: CSIM_ERR_CONFIG).  y, s [B][F][P][P] complex; s may be NULL.                           */
int  csim_sp_batch(csim_engine* eng, const double* params, int32_t B, const double* freqs, int32_t F, double* y,
                   double* s, uint32_t* status);

/* ---- Two-port noise analysis (.SP ... 1; Y, the port noise-current correlation matrix Cy and, for two ports, NF,
 *      NFmin, Rn and Yopt by one adjoint factorisation per frequency) ----
 * Card: `.SP DEC|OCT|LIN n fstart fstop 1`, ngspice's donoise; the token only records the wish
 *   (csim_netlist_sp_noise), the entry points below work with or without it.
 * System.  For instance b and angular frequency w, A = G + j w C is exactly the matrix of "AC analysis": the same
 *   assembly, the same elements left out.  Ports are those of "S-parameter analysis", k_i the branch equation of port
 *   i; generators those of "Noise analysis": the same elements, the same PSD formulas at temp_k.
 * Adjoint multi-RHS solve.  A^T L = [e_{k_1} ... e_{k_P}], real unit vectors, with the transposed load of "Noise
 *   analysis" (A^T(i,j) = G(j,i) + j (w C(j,i)), w C one product) and the multi-RHS algorithm of "S-parameter
 *   analysis"; pivoting never looks at a right-hand side.  lambda_i is column i.  A column maximum below lu_eps^2:
 *   every output of that (instance, frequency) is +0.0, CSIM_ST_LU_TINY_PIVOT is OR-ed into the status, the sweep
 *   goes on.
 * Y(i,j) = -lambda_i[k_j], both parts negated.  Mathematically the Y of csim_sp_batch; numerically it comes from the
 *   factorisation of the transposed matrix, so its low bits may differ from csim_sp_batch's.
 * Cy.  Per generator s between equations (a_s, b_s): t_i = lambda_i[a_s] - lambda_i[b_s] (ground = (0, 0)).  For
 *   i <= j:  q.re = (t_i.re t_j.re + t_i.im t_j.im) psd_s,  q.im = (t_i.im t_j.re - t_i.re t_j.im) psd_s.
 *   Cy(i,j) = 0.0 + q(0) + q(1) + ... in ascending s, re and im separately; Cy(j,i) = conj(Cy(i,j)) (im negated).
 *   The diagonal sums the real part alone and its imaginary part is +0.0: Cy(i,i).re is bit for bit the onoise of
 *   "Noise analysis" taken with the output at k_i.  A^2/Hz, one-sided.
 * Noise parameters, P == 2 only, port 1 the input and port 2 the output; all linear (decibels are the caller's).
 *   kT4_0 = 4.0 * 1.380649e-23 * 290.0 (the IEEE reference temperature, whatever temp_k) and Gs = 1.0 / Z0_1 are
 *   computed once on the host.  Every real division below is x * (1.0 / y), complex ones the AC division:
 *     d = Y21.re Y21.re + Y21.im Y21.im     r = Y11 / Y21     Cvv = Cy22.re * (1 / d)
 *     Cii = (Cy11.re - 2.0 * (r.re Cy12.re + r.im Cy12.im)) + (r.re r.re + r.im r.im) * Cy22.re
 *     q = (Cy12.re - r.re Cy22.re,  r.im Cy22.re - Cy12.im) / Y21        (Cvi = -q)
 *     Gcor = (-q.re) * (1 / Cvv)    Bcor = q.im * (1 / Cvv)              (Ycor = conj(Cvi) / Cvv)
 *     Rn = Cvv * (1 / kT4_0)        Gu = (Cii - (Gcor Gcor + Bcor Bcor) * Cvv) * (1 / kT4_0)
 *     Gopt = sqrt(max0(Gu * (1 / Rn) + Gcor Gcor)), max0(x) = x < 0.0 ? 0.0 : x (a NaN passes through)
 *     Yopt = (Gopt, -Bcor)          Fmin = 1.0 + (2.0 * Rn) * (Gcor + Gopt)
 *     NF = 1.0 + (Gu + Rn * ((Gs + Gcor) (Gs + Gcor) + Bcor Bcor)) * (1 / Gs)
 *   Cvv not > 0.0 (a noiseless or purely current-noisy two-port): Rn = +0.0, Yopt = (+0.0, +0.0), Fmin = 1.0,
 *   NF = 1.0 + (Cii * (1 / kT4_0)) * (1 / Gs).  Y21 == 0 gets no special case: the outputs are what IEEE arithmetic
 *   gives.  The exact order of every operation: engine/ac_port_noise.hpp, written once for host and device.
 * No FMA contraction anywhere.  Circuits of up to 63 unknowns (CSIM_ERR_UNSUPPORTED beyond); no port or a bad port
 * numbering: CSIM_ERR_CONFIG; temp_k <= 0 or not finite: CSIM_ERR_CONFIG; a non-NULL noise-parameter pointer with
 * P != 2: CSIM_ERR_CONFIG.  S == 0 is legal: Cy = 0.
 *
 * Enqueues the sweep; never waits for it; frequency lists as csim_ac_batch_dev (same buffers, same discipline).
 *   d_y, d_cy [F][P][P][B] complex (re, im), row i then column j, instance fastest
 *   d_nf, d_fmin, d_rn [F][B]    d_yopt [F][B] complex    d_status [B], OR-ed
 * Every output but d_cy may be NULL (the Python binding's noise_params=False passes NULL for the four noise
 * parameters).  The engine option ac_kernel picks the kernel as for AC; both give bit-identical
 * results.                                                                                                        */
int  csim_spnoise_batch_dev(csim_engine* eng, const double* d_params /*[P][B]*/, int32_t B, const double* d_xop,
                            const double* freqs, int32_t F, double temp_k, double* d_y, double* d_cy, double* d_nf,
                            double* d_fmin, double* d_rn, double* d_yopt, uint32_t* d_status, void* stream);
/* DC operating point, then the sweep.  params [B][P] or NULL (nominal); freqs NULL = the grid of the netlist's .SP
 * card (F ignored; no card: CSIM_ERR_CONFIG).  y, cy [B][F][P][P] complex; nf, fmin, rn [B][F]; yopt [B][F] complex;
 * every output but cy may be NULL.                                                                                */
int  csim_spnoise_batch(csim_engine* eng, const double* params, int32_t B, const double* freqs, int32_t F,
                        double temp_k, double* y, double* cy, double* nf, double* fmin, double* rn, double* yopt,
                        uint32_t* status);

/* ---- Distortion analysis (.DISTO; single-tone harmonic distortion HD2, HD3 by a Volterra series at the operating
 *      point: three factorisations per frequency) ----
 * Card: `.DISTO V(out[,ref]) DEC|OCT|LIN n fstart fstop`, the output as on .NOISE, the grid of csim_ac_freqs.  Single
 *   tone only: a further token (ngspice's f2overf1) is a card error, reported, the statement dropped.
 * System.  For instance b and angular frequency w, A(w) = G + j w C is exactly the matrix of "AC analysis" above: the
 *   same assembly, the same elements left out, tran_gmin.  J is that section's right-hand side: `AC mag [phase]` of the
 *   netlist's sources, mag a PEAK amplitude that matters here (x2 ~ mag^2, x3 ~ mag^3).  No source with mag != 0:
 *   CSIM_ERR_CONFIG.
 * Non-linearity.  The only one of this simulator is the level-1 MOSFET drain current (the Cj0 capacitances are
 *   constants).  Inside a region it is a polynomial of degree <= 3 in (Vgs, Vds), so its expansion to third order is
 *   exact.  Devices are the MOSFETs in element order, M per circuit (csim_netlist_disto_device), each with its drain,
 *   gate and source equations (d, g, s), -1 for ground.
 * Coefficients, seven per (device, instance), computed once at x_op.  With mos_eval's own quantities and comparisons
 *   (p = -1.0 for a PMOS, else 1.0; Vgs = p * (Vg - Vs); Vds = p * (Vd - Vs); on when Vgs > Vth && Vds >= 0.0;
 *   Vov = Vgs - Vth; triode when Vds < Vov; factor = 1.0 + lambda * Vds), every product and sum below one operation
 *   in the order written:
 *     off, or factor < 0.0 (mos_eval clamps it to 0): all seven +0.0
 *     saturation  gg = K * factor    gd = (K * Vov) * lambda    ggd = K * lambda    dd = ggg = gdd = ddd = 0.0
 *     triode      gd = K * factor + (K * Vds) * lambda          dd = 2.0 * ((K * (Vov - Vds)) * lambda) - K * factor
 *                 gdd = 2.0 * (K * lambda)    ddd = -3.0 * (K * lambda)             gg = ggg = ggd = 0.0
 *   These are the derivatives of the current in the device's effective coordinates.  In physical coordinates
 *   (Ug = Vg - Vs, Ud = Vd - Vs, current drain -> source) the three second-order ones are multiplied by p
 *   (c_gg = p * gg, c_gd = p * gd, c_dd = p * dd: a zero among them is -0.0 for a PMOS), the four third-order ones are
 *   unchanged (p p^3 = 1).  Order in a coefficient table: c_gg, c_gd, c_dd, c_ggg, c_ggd, c_gdd, c_ddd.
 * Complex arithmetic.  A product of two complex values is four real products, then one difference (re) and one sum
 *   (im), as in "AC analysis"; a real factor times a complex value scales re and im, one product each; sums of complex
 *   values add re and im separately, left to right.  No FMA contraction anywhere.
 * Order 1.  A(w) x1 = J, the AC solve.
 * Order 2.  Per device m: Ug = x1[g] - x1[s], Ud = x1[d] - x1[s], ground = (0, 0);
 *     I2 = 0.5 * ( ((0.5 * c_gg) * (Ug Ug) + c_gd * (Ug Ud)) + (0.5 * c_dd) * (Ud Ud) ).
 *   Right-hand side: every entry starts at +0.0; the devices are taken in ascending order; each subtracts I2 at d, then
 *   adds it at s (ground: no entry).  A(2.0 * w) x2 = rhs2.
 * Order 3.  With Ug2, Ud2 taken from x2 the same way, GG = Ug Ug and DD = Ud Ud:
 *     a = (((c_ggg / 6.0) * (GG Ug) + (0.5 * c_ggd) * (GG Ud)) + (0.5 * c_gdd) * (Ug DD)) + (c_ddd / 6.0) * (DD Ud)
 *     b = (c_gg * (Ug Ug2) + c_gd * ((Ug Ud2) + (Ud Ug2))) + c_dd * (Ud Ud2)
 *     I3 = 0.25 * a + 0.5 * b
 *   accumulated like I2.  A(3.0 * w) x3 = rhs3.
 * Outputs.  The three phasor vectors, and for the output V(out_p[, out_m]): v_k = x_k[out_p] - x_k[out_m],
 *   |z| = sqrt(z.re z.re + z.im z.im), HD2 = |v2| / |v1|, HD3 = |v3| / |v1| (true divisions); +0.0 where |v1| == 0.
 *   out_p == out_m or out_p < 0: CSIM_ERR_ARG.
 * Failures.  A column maximum below lu_eps^2 at order k makes x_k and every higher order +0.0 (their HD too) and sets
 *   CSIM_ST_LU_TINY_PIVOT; the sweep goes on.  All three factorisations are attempted whatever M is, so the flags do
 *   not depend on the device list.  M == 0 is legal: x2 = x3 = 0.
 * Circuits of up to 63 unknowns (CSIM_ERR_UNSUPPORTED beyond); ac_kernel=block: CSIM_ERR_UNSUPPORTED (the block shape
 * covers AC and noise analysis only).  The exact order of every operation: engine/ac_disto.hpp, written once for host
 * and device.
 *
 * Enqueues the sweep; never waits for it; frequency lists as csim_ac_batch_dev (same buffers, same discipline).
 *   d_h [F][3][N][B] complex (re, im): x1, x2, x3, or NULL    d_hd [F][2][B]: HD2, HD3
 *   d_coef [M][7][B] or NULL: the coefficients                d_status [B], OR-ed
 * The engine option ac_kernel picks the kernel as for AC (wave, N <= 63; packed, N <= 32); both give bit-identical
 * results.                                                                                                        */
/* .DISTO card: output equations (out_m_eq -1: ground; -2: a node the netlist does not have), the sweep as for .AC */
int  csim_netlist_disto(const csim_netlist* nl, int32_t* enabled, int32_t* out_p_eq, int32_t* out_m_eq, int32_t* sweep,
                        int32_t* n_points, double* fstart, double* fstop);
/* The non-linear devices, in element order: element index and the drain, gate and source equations (-1: ground) */
int  csim_netlist_num_disto_devices(const csim_netlist* nl);
int  csim_netlist_disto_device(const csim_netlist* nl, int32_t i, int32_t* elem, int32_t* eq_d, int32_t* eq_g,
                               int32_t* eq_s);
int  csim_disto_batch_dev(csim_engine* eng, const double* d_params /*[P][B]*/, int32_t B, const double* d_xop,
                          const double* freqs, int32_t F, int32_t out_p_eq, int32_t out_m_eq, double* d_h, double* d_hd,
                          double* d_coef, uint32_t* d_status, void* stream);
/* DC operating point, then the sweep.  params [B][P] or NULL (nominal); freqs NULL = the grid of the netlist's .DISTO
 * card (F ignored); out_p_eq == -2 = the card's output (out_m_eq ignored); no card: CSIM_ERR_CONFIG.
 * h [B][F][3][N] complex or NULL; hd [B][F][2]; coef [B][M][7] or NULL.                                             */
int  csim_disto_batch(csim_engine* eng, const double* params, int32_t B, const double* freqs, int32_t F,
                      int32_t out_p_eq, int32_t out_m_eq, double* h, double* hd, double* coef, uint32_t* status);

/* ---- Intermodulation analysis (.IMD; two-tone IM2 and IM3 by a Volterra series at the operating point: six
 *      factorisations per tone pair) ----
 * Card: `.IMD V(out[,ref]) DEC|OCT|LIN n fstart fstop f2overf1`, the output as on .DISTO.  f1 sweeps the grid of
 *   csim_ac_freqs; f2 stays at f2overf1 * fstart (ngspice's rule), 0 < f2overf1 < 1, so f1 > f2 > 0 at every point.
 *   Any other token count or an f2overf1 outside (0, 1) is a card error, reported, the statement dropped.
 * System, devices, coefficients c, complex arithmetic, right-hand side accumulation: those of "Distortion analysis".
 *   x(t) = Re sum X e^{jwt}, peak amplitudes.  Both tones drive the netlist's `AC mag [phase]` sources (J2 = J1, the
 *   equal-amplitude two-tone test); distinct excitations exist only in csim_imd_solve_batch.
 * Forms.  A "pair" U = (Ug, Ud) of a solution x and a device is (x[g] - x[s], x[d] - x[s]); * is the conjugate.
 *     Q(A, B)    = 0.5 * ( (c_gg * (Ag Bg) + c_gd * ((Ag Bd) + (Ad Bg))) + c_dd * (Ad Bd) )
 *     T(A, A, B) = ( ((c_ggg * (GG Bg) + c_ggd * ((GG Bd) + 2.0 * (GD Bg))) + c_gdd * (2.0 * (GD Bd) + (DD Bg)))
 *                    + c_ddd * (DD Bd) ) / 6.0,        GG = Ag Ag, GD = Ag Ad, DD = Ad Ad
 * Six solves per point, in this order; Ua, Ub, Vd, Vh are the pairs of x0, x1, x3, x4.  The current of each device is
 *   subtracted at d and added at s, the devices in ascending order.
 *     k  frequency                right-hand side
 *     0  w1                       J1
 *     1  w2                       J2
 *     2  ws = w1 + w2             Q(Ua, Ub)
 *     3  wd = w1 - w2             Q(Ua, Ub*)
 *     4  wh = 2.0 * w1            0.5 * Q(Ua, Ua), computed as I2 of "Distortion analysis"
 *     5  w3 = wh - w2             (0.75 * T(Ua, Ua, Ub*) + Q(Ua, Vd)) + Q(Ub*, Vh)
 *   A(-w) = G - j w C is ordinary arithmetic: any finite (w1, w2) is legal in the direct entry.
 * Outputs.  The six solutions, and v_k = x_k[out_p] - x_k[out_m]: IM2+ = |v2| / |v0|, IM2- = |v3| / |v0|,
 *   IM3 = |v5| / |v0|, |.| and the division as HD2, HD3: +0.0 where |v0| == 0.  The output intercept amplitude
 *   OIP3 = |v0| * sqrt(|v0| / |v5|) is left to the caller.
 * Failures.  All six factorisations are attempted; a failed solve makes itself and every later one +0.0 and sets
 *   CSIM_ST_LU_TINY_PIVOT.  M == 0 is legal.
 * Sizes and kernels as "Distortion analysis"; both kernel shapes give bit-identical results.  The exact order of every
 * operation: engine/ac_imd.hpp, written once for host and device.
 *
 * Enqueues the sweep; never waits for it; frequency lists as csim_ac_batch_dev.  freqs [F]: f1 in Hz; f2 in Hz, finite.
 *   d_h [F][6][N][B] complex (re, im): x0 .. x5, or NULL      d_im [F][3][B]: IM2+, IM2-, IM3
 *   d_coef [M][7][B] or NULL: the coefficients                d_status [B], OR-ed                                  */
/* .IMD card: as csim_netlist_disto, then f2overf1 */
int  csim_netlist_imd(const csim_netlist* nl, int32_t* enabled, int32_t* out_p_eq, int32_t* out_m_eq, int32_t* sweep,
                      int32_t* n_points, double* fstart, double* fstop, double* f2overf1);
int  csim_imd_batch_dev(csim_engine* eng, const double* d_params /*[P][B]*/, int32_t B, const double* d_xop,
                        const double* freqs, int32_t F, double f2, int32_t out_p_eq, int32_t out_m_eq, double* d_h,
                        double* d_im, double* d_coef, uint32_t* d_status, void* stream);
/* DC operating point, then the sweep.  params [B][P] or NULL (nominal); freqs NULL = the grid and the f2 of the
 * netlist's .IMD card (F and f2 ignored); out_p_eq == -2 = the card's output (out_m_eq ignored); no card:
 * CSIM_ERR_CONFIG.  h [B][F][6][N] complex or NULL; im [B][F][3]; coef [B][M][7] or NULL.                           */
int  csim_imd_batch(csim_engine* eng, const double* params, int32_t B, const double* freqs, int32_t F, double f2,
                    int32_t out_p_eq, int32_t out_m_eq, double* h, double* im, double* coef, uint32_t* status);

/* ---- Loop-gain analysis (.STB; the loop gain T of a feedback loop by Middlebrook's double injection at a V source in
 *      series in the loop, one factorisation with two right-hand sides per frequency; phase and gain margins) ----
 * Card: `.STB Vprobe DEC|OCT|LIN n fstart fstop`, the grid of csim_ac_freqs.  Any other token count is a card error,
 *   reported, the statement dropped.  The card changes nothing in the IR.  A name the netlist does not have keeps the
 *   card, with element -2, refused when used (CSIM_ERR_CONFIG).
 * Probe.  A V source of the netlist in series in the loop, normally DC 0.  Its + node is the side that DRIVES the loop
 *   (equation x), its - node the side that RECEIVES (equation y); k is its branch equation, the branch current flowing
 *   from + through the source ("S-parameter analysis").  With reverse transmission T depends on this orientation.
 *   Not a V source, a node on ground, or + and - on one node: CSIM_ERR_CONFIG.
 * System.  For instance b and angular frequency w, A(w) = G + j w C is exactly the matrix of "AC analysis" above.  Every
 *   AC stimulus of the netlist is ignored: J is not read, and no source needs an AC magnitude.
 * Two columns, one factorisation.
 *   Column 0, voltage injection: the real unit vector at row k, exactly a port column of "S-parameter analysis".
 *     vx = X0[x], vy = X0[y].
 *   Column 1, current injection: +1.0 (im +0.0) at row x, nothing else.  SIGN: this is the column the AC assembly leaves
 *     for `Iinj 0 <+node> AC 1` beside a probe with AC 0 -- an I source `I n1 n2` stamps J(n1) -= I and J(n2) += I, so
 *     1 A from ground into the + node is +1.0 at x.  ib = X1[k], the part of that ampere that flows through the probe.
 * Loop gain.  Tv = -vx / vy, Ti = (1 - ib) / ib, T = (Tv Ti - 1) / (Tv + Ti + 2), evaluated without the intermediate
 *   divisions, in this order:
 *     a = 1.0 - ib,  b = 1.0 + ib                 (re: 1.0 -/+ ib.re; im: 0.0 -/+ ib.im)
 *     num = -(vx a) - (vy ib)                     (each part: the exact negation of the first product minus the second)
 *     den =  (vy b) - (vx ib)
 *     T   = num / den                             (as a * conj(p) * (1 / |p|^2), "AC analysis")
 *   Products of complex values as in "AC analysis" (four real products, one difference, one sum).  No FMA contraction.
 *   T is positive real at low frequency for negative feedback.
 * Failures.  A fails its pivot test (a column maximum below lu_eps^2): both solutions +0.0, T = +0.0 + 0.0j,
 *   CSIM_ST_LU_TINY_PIVOT.  den exactly zero: the same T and flag.  The sweep goes on.
 * Margins (optional), per instance, from T_0 .. T_{F-1} at strictly increasing positive frequencies f_k in Hz (anything
 *   else with margins asked for: CSIM_ERR_ARG).  pi = 3.14159265358979323846; atan2, log10, log, exp of the C library
 *   of the side that runs (the device's on the device), so margins are not bit-exact across implementations.
 *     m_k = re^2 + im^2 of T_k,  g_k = 10.0 * log10(m_k)
 *     phi_0 = atan2(im, re);  d_k = atan2 of T_k * conj(T_{k-1});  phi_k = phi_{k-1} + d_k  (unwrapped by increments)
 *     unity crossing: the smallest k >= 1 with m_{k-1} >= 1.0 > m_k:
 *       t = g_{k-1} / (g_{k-1} - g_k);  fc = f_{k-1} * exp(t * log(f_k / f_{k-1}));
 *       PM = 180.0 + ((phi_{k-1} + t * d_k) * 180.0) / pi
 *     phase crossing: the smallest k >= 1 with phi_{k-1} > -pi >= phi_k:
 *       t = (phi_{k-1} + pi) / (phi_{k-1} - phi_k);  f180 by the same interpolation;
 *       GM = -(g_{k-1} + t * (g_k - g_{k-1}))
 *   The walk ends at the first T_k that is exactly zero or not finite; what was found before it stays.
 *   margins = PM (degrees), fc (Hz), GM (dB), f180 (Hz); a pair that is not found is NaN.  found: bit 0 the unity
 *   crossing, bit 1 the phase crossing.
 * Circuits of up to 63 unknowns (CSIM_ERR_UNSUPPORTED beyond); ac_kernel=block: CSIM_ERR_UNSUPPORTED.  The exact order
 * of every operation: engine/ac_stb.hpp, written once for host and device.
 * Order of the refusals of an engine's call: a bad argument (margins on a grid that does not increase among them);
 *   ac_kernel=block; more than 63 unknowns; no card where the probe was left to it; the probe (not in the netlist, not a
 *   V source, a node on ground, + and - on one node -- its branch equation is never a node's, so three different
 *   equations follow); ac_kernel=packed above 32 unknowns.  csim_stb_batch with freqs NULL asks for the card's grid
 *   before any of these but its own argument check.
 *
 * Enqueues the sweep and (d_margins given) the margins kernel after its last chunk; never waits; frequency lists as
 * csim_ac_batch_dev.  probe_elem: element index of the probe, -1 = the .STB card's (no card: CSIM_ERR_CONFIG).
 *   d_t [F][B] complex (re, im)                d_x [F][2][N][B] complex or NULL: the two solutions
 *   d_margins [4][B] or NULL                   d_found [B] int32 or NULL (needs d_margins)        d_status [B], OR-ed
 * The engine option ac_kernel picks the kernel as for AC (wave, N <= 63; packed, N <= 32); both give bit-identical T.  */
/* .STB card: the probe's element index (-2: a name the netlist does not have), the equations of its + node, - node and
 * branch (-1: ground; all -2 when the probe is not a V source), the sweep as for .AC */
int  csim_netlist_stb(const csim_netlist* nl, int32_t* enabled, int32_t* elem, int32_t* eq_p, int32_t* eq_m, int32_t* eq_br,
                      int32_t* sweep, int32_t* n_points, double* fstart, double* fstop);
int  csim_stb_batch_dev(csim_engine* eng, const double* d_params /*[P][B]*/, int32_t B, const double* d_xop,
                        const double* freqs, int32_t F, int32_t probe_elem, double* d_t, double* d_x, double* d_margins,
                        int32_t* d_found, uint32_t* d_status, void* stream);
/* DC operating point, then the sweep.  params [B][P] or NULL (nominal); freqs NULL = the grid of the netlist's .STB card
 * (F ignored).  t [B][F] complex; x [B][F][2][N] complex or NULL; margins [B][4] or NULL; found [B] or NULL.          */
int  csim_stb_batch(csim_engine* eng, const double* params, int32_t B, const double* freqs, int32_t F, int32_t probe_elem,
                    double* t, double* x, double* margins, int32_t* found, uint32_t* status);

/* ---- Pole analysis (.PZ POL; the natural frequencies of every instance's linearisation, without a frequency grid) ----
 * Card: `.PZ POL fmax [sigma0]`, SPICE number suffixes, either case.  `.PZ ZER ...` and `.PZ PZ ...` are reported as
 *   `Line n: .PZ supports POL only: <line>` and dropped: zeros need a deflation of the infinite structure that is not
 *   here.  Any other token count is a card error, reported, the statement dropped.  A later valid card replaces an
 *   earlier one.  The card changes nothing in the IR.
 * System.  G and C of instance b exactly as in "AC analysis".  The poles are the s with det(G + s C) = 0.  Two real
 *   scalars: fmax > 0 in Hz, sigma0 in rad/s (default 0.0).  All arithmetic is real; no FMA contraction; sqrt is the only
 *   library function, so host and device compute the same bits.
 * 1. A0 = G + sigma0 * C, one product and one sum per entry.
 * 2. M = -A0^-1 C by a real LU with partial pivoting on [A0 | C], the N columns of C as right-hand sides: pivot = the
 *    largest |a| of the column, the lowest row on ties, a NaN diagonal keeps the pivot; multiplier a / pivot; rows whose
 *    entry in the pivot column is exactly zero are skipped; back substitution per column, the products U(i,l) x(l)
 *    subtracted for l ascending, zero U(i,l) skipped, then the division by U(i,i); then the exact negation.  A column
 *    maximum below lu_eps: CSIM_ST_PZ_SINGULAR, n_poles = 0, every pole slot NaN + NaN j.
 * 3. The eigenvalues mu of M by the EISPACK chain:
 *    balance  diagonal similarity by powers of two.  SWEEP ORDER: Gauss-Seidel -- the indices i = 0 .. N-1 in order,
 *             each with c = sum |M(j,i)| and r = sum |M(i,j)| over j != i, j ascending, of the matrix as the indices
 *             before it left it; c or r zero (or not finite): nothing; else f = 1, g = r / 2, while c < g: f *= 2,
 *             c *= 4; g = r * 2, while c > g: f /= 2, c /= 4; if (c + r) / f < 0.95 * (c0 + r): row i times 1 / f, then
 *             column i times f.  Sweeps repeat until one changes nothing, AT MOST 16 of them.
 *    elmhes   for m = 1 .. N-2: pivot = the largest |a(j,m-1)|, j = m .. N-1, the lowest index on ties (all zero: the
 *             column is skipped); rows, then columns, m and the pivot's exchanged; y(i) = a(i,m-1) / a(m,m-1) kept in
 *             place (zero entries stay); first every a(i,j) -= y(i) a(m,j) (i > m, j >= m), then every
 *             a(j,m) += y(i) a(j,i) (all j; i ascending; zero y(i) skipped).  Then +0.0 below the subdiagonal.
 *    hqr      Francis double-shift QR with deflation, as EISPACK hqr: the exact tests |h(l,l-1)| + s == s with
 *             s = |h(l-1,l-1)| + |h(l,l)| (anorm when that is zero; anorm = the sum over the rows, ascending, of each
 *             row's sum of |h(i,j)|, j = max(i-1,0) .. N-1 ascending); exceptional shifts at iterations 10 and 20; at
 *             most 30 iterations per eigenvalue, then CSIM_ST_PZ_NONCONV, n_poles = 0, NaN slots.  Per bulge step the
 *             row phase (columns k .. nn) is finished before the column phase (rows l .. min(nn, k+3)) starts.  The
 *             routine always terminates, after at most 30 N sweeps.
 * 4. Cut.  wmax = 2 pi fmax (pi = 3.14159265358979323846).  An eigenvalue is a finite pole iff
 *    (mur^2 + mui^2) * wmax^2 >= 1.0; everything else is a pole at infinity and dropped.  LIMIT: the cut is the only
 *    thing that separates them.  Eigenvalues mu = 0 that belong to Jordan blocks come out near sqrt(eps) ||M||, not near
 *    eps ||M||, so no rank rule finds them: choose fmax well above the fastest pole of interest and well below
 *    1 / (2 pi sqrt(eps) ||M||); a true pole faster than fmax is dropped with them.
 * 5. Pole s = sigma0 + conj(mu) / (mur^2 + mui^2): re = sigma0 + mur / m2, im = (0.0 - mui) / m2.  Order: descending
 *    m2, then descending Im mu, then descending Re mu, then the eigenvalue's index.  The dominant (slowest) pole is
 *    first; a conjugate pair is adjacent, the member with Im mu > 0 (Im s < 0) first.  Slots n_poles .. N-1 are
 *    NaN + NaN j.
 * 6. Summary per instance: n_poles; n_rhp, the count with Re s > 0.0; max_re, the largest Re s (NaN when n_poles == 0).
 * Circuits of up to 63 unknowns (CSIM_ERR_UNSUPPORTED beyond).  One kernel, one wavefront per instance: ac_kernel=block
 * and ac_kernel=packed are CSIM_ERR_UNSUPPORTED.  The exact order of every operation: engine/pz.hpp, written once for
 * host and device.  Results do not depend on B or on how the batch is chunked.
 * Order of the refusals of an engine's call: a bad argument (fmax not finite or <= 0, sigma0 not finite: CSIM_ERR_ARG);
 *   ac_kernel=block or packed; more than 63 unknowns; no card where fmax was left to it (fmax NaN: CSIM_ERR_CONFIG).
 *
 * Enqueues and never waits.  fmax NaN: the .PZ card's fmax and sigma0.
 *   d_poles [N][B] complex (re, im): slot k of instance b       d_n_poles, d_n_rhp [B] int32       d_max_re [B]
 *   d_status [B], OR-ed                                                                                             */
int  csim_netlist_pz(const csim_netlist* nl, int32_t* enabled, double* fmax, double* sigma0);
int  csim_pz_batch_dev(csim_engine* eng, const double* d_params /*[P][B]*/, int32_t B, const double* d_xop, double fmax,
                       double sigma0, double* d_poles, int32_t* d_n_poles, int32_t* d_n_rhp, double* d_max_re,
                       uint32_t* d_status, void* stream);
/* DC operating point, then the poles.  params [B][P] or NULL (nominal).  poles [B][N] complex; n_poles, n_rhp, max_re,
 * status [B], each optional.                                                                                        */
int  csim_pz_batch(csim_engine* eng, const double* params, int32_t B, double fmax, double sigma0, double* poles,
                   int32_t* n_poles, int32_t* n_rhp, double* max_re, uint32_t* status);

/* ---- Periodic steady state (.HB f0 nharm; the reference parses the card and its steady-state source is empty) ----
 * The periodic steady state of this engine's own backward-Euler transient, found by shooting Newton, and the harmonics
 * 0 .. n_harm of the probes, for every instance of the batch.
 *   h = tstep, T = 1 / f0, K = round(T / h) (csim_pss_num_steps).  PHI maps a state x at step 0 to the state after steps
 *   1 .. K of csim_tran_batch_dev (step_first = 0, t_k = k h) on the general kernel: the reference's damped Newton with
 *   tran_alpha, tran_tol, tran_max_iters, tran_gmin, histories from the previous state; x is the whole state.
 * Per instance the analysis returns
 *   x0       with || PHI(x0) - x0 ||_inf < tol
 *   X[m][p]  m = 0 .. n_harm, probes p: X[0] = (1/K) sum_{k=1..K} x_k[p] (imaginary part 0);
 *            X[m] = (2/K) sum_{k=1..K} x_k[p] (c[(m k) mod K] - j s[(m k) mod K]) for m >= 1, with the table
 *            c[j] = cos(2 pi j / K), s[j] = sin(2 pi j / K) made once on the host in double (csim_pss_twiddles) and
 *            x_k the K steps that start at the returned x0.  Peak phasors, cosine reference at t = 0:
 *            x(t) ~ Re sum_m X[m] e^{j m 2 pi f0 t}, the convention of the distortion analysis.  Real and imaginary sums
 *            are accumulated separately, k ascending, every product and sum rounded on its own (no FMA contraction); the
 *            scale (1/K or 2/K, one division) multiplies the finished sum.  A numpy loop over the same table gives
 *            the same bits.
 *   rounds   shooting rounds used, and status.
 * Sources are evaluated exactly as the transient's first period evaluates them (t = k h, k = 1 .. K); the analysis answers
 * for their periodic extension.  A SIN source's fourth number is a delay in seconds, so a source whose delay lies beyond
 * the first period is a constant to the analysis, as it is to the transient there.  A waveform whose first period does
 * not join itself (a delayed start inside the period, a PULSE of another period) is the caller's business: the analysis
 * runs and answers for that period repeated.
 * One shooting round: integrate one period from x0, carrying W_k = J_k^-1 (Hm W_{k-1}), W_0 = I, where J_k is the
 * transient matrix assembled at the converged iterate of step k and Hm = d(right-hand side)/d(x_prev), which depends on
 * the parameters and h only; r = x_K - x0; ||r||_inf < tol: the instance is done, its x0 is kept and this round's
 * harmonics are its result; otherwise (I - W_K) d = r by the engine's real LU and x0 += d.  The first x0 is the caller's
 * (normally the DC operating point).
 * Rounds: a circuit without state closes in one round, a linear circuit in two PROVIDED what the first update leaves is
 * below tol -- each step's truncated damped iteration leaves up to (1 - tran_alpha) / tran_alpha * tran_tol = 1.22e-6
 * whose direction follows the trajectory, and a resonant circuit carries it to x_K amplified (a series RLC of Q = 7:
 * 2.6e-5, a third round); after that the closure falls quadratically (DESIGN.md 8h has the table).
 * Status: the transient's own bits are OR-ed in as the transient does.  CSIM_ST_PSS_NONCONV: max_rounds reached; x0 and
 * the harmonics of the last round are still written (that x0 is the start of the period the harmonics describe).
 * CSIM_ST_PSS_SINGULAR: a tiny pivot in I - W_K or in a step's sensitivity solve; the instance stops.  An instance whose
 * start vector or trajectory is not finite stops with CSIM_ST_TRAN_NONFINITE and disturbs no other.
 * Refused before anything looks at the device: null pointers, B <= 0, n_harm < 0, numbers that are not finite, a probe
 * equation out of range: CSIM_ERR_ARG; no f0 and no .HB card (no tstep and no .TRAN card): CSIM_ERR_CONFIG;
 * |K h f0 - 1| > 1e-9, K < 2 n_harm + 1 or K > 2^22 (the cap bounds the table and keeps the step time's int cast
 * safe; buffer.sp's own card, .hb 1e-2 3 at its .TRAN step, falls under it): CSIM_ERR_CONFIG; more than 63 unknowns:
 * CSIM_ERR_UNSUPPORTED.
 * csim_pss_batch_dev: probe_eq host [n_probe] or NULL = every unknown; tol, max_rounds <= 0: the engine options pss_tol,
 * pss_max_rounds.  d_x0 [N][B] in: start, out: steady state; d_harm [n_harm+1][n_probe][B] complex; d_rounds [B];
 * d_status [B], OR-ed.  It runs at most max_rounds rounds and after each reads back one counter of unfinished instances,
 * so UNLIKE THE SWEEPS THIS ENTRY WAITS ON THE STREAM; it returns with the results complete.
 * csim_pss_batch: DC operating point first.  params [B][P] or NULL (nominal); tstep <= 0: the .TRAN card's step;
 * f0 <= 0: the .HB card's f0 and n_harm; x0_out [B][N] or NULL; harm_out [B][n_harm+1][n_probe] complex; rounds, status
 * [B] or NULL.  Engine options: pss_tol (2e-6: what a step's stopping rule may leave of its own Newton iteration,
 * (1 - tran_alpha) / tran_alpha * tran_tol = 1.22e-6, rounded up; the transient's measured period-to-period floor lies far
 * below it), pss_max_rounds (20, a cap), pss_chunk (test aid: instances per chunk of the W_K scratch,
 * 0 = ac_chunk).  The exact order of every operation the analysis adds to the transient: engine/pss.hpp. */
int  csim_netlist_hb(const csim_netlist* nl, int32_t* enabled, double* f0, int32_t* n_harm);
int64_t csim_pss_num_steps(double tstep, double f0);            /* K, or < 0: CSIM_ERR_ARG / CSIM_ERR_CONFIG */
int  csim_pss_twiddles(int64_t K, double* cos_out /*[K]*/, double* sin_out /*[K]*/);
int  csim_pss_batch_dev(csim_engine* eng, const double* d_params /*[P][B]*/, int32_t B, double tstep, double f0,
                        int32_t n_harm, const int32_t* probe_eq /*host*/, int32_t n_probe, double tol, int32_t max_rounds,
                        double* d_x0 /*[N][B]*/, double* d_harm, int32_t* d_rounds, uint32_t* d_status, void* stream);
int  csim_pss_batch(csim_engine* eng, const double* params, int32_t B, double tstep, double f0, int32_t n_harm,
                    const int32_t* probe_eq, int32_t n_probe, double tol, int32_t max_rounds, double* x0_out,
                    double* harm_out, int32_t* rounds, uint32_t* status);

/* ---- Periodic AC analysis (.PAC): the backward-Euler transient linearised around a periodic orbit ----
 * A small tone a e^{j 2 pi f t} on the netlist's `AC mag [phase]` sources, superposed on the large-signal orbit of
 * "Periodic steady state", appears at every f + m f0: a mixer's conversion gain is the transfer to m = -1.  None of the
 * analyses that linearise at a DC point can translate frequency; this one linearises the transient's step around the orbit.
 * Carried over from the periodic steady state: h = tstep, f0, K = csim_pss_num_steps(h, f0), the table c[j], s[j].
 * Orbit: the states x_1 .. x_K of K steps of the general transient from the given x0, integrated with the same device
 *   functions in the same order as the periodic steady state's period, hence the same bits.  J_k is the transient matrix
 *   assembled at the converged x_k (one more MOSFET pass and assembly), Hm = d(right-hand side)/d(x_prev) as there.
 * Excitation: u, complex [N], is the right-hand side of the AC analysis: the source slots carry mag (cos, sin)(phase),
 *   every history is zero.
 * Frequency constants, for an input frequency f > 0, made on the host in double: z = cos(theta) - j sin(theta),
 *   theta = 2 pi f h; z_K = cos(theta_K) - j sin(theta_K), theta_K = 2 pi (f / f0 - floor(f / f0)); z_K is not z powered.
 * Recursion: with the perturbation written as dx_k = e^{j 2 pi f t_k} p_k, p periodic,
 *     J_k p_k = z (Hm p_{k-1}) + u,  k = 1 .. K.
 *   Operation order: q = Hm p_{k-1} row by row over the non-zero Hm(i, l), l ascending, product and sum rounded
 *   separately, real and imaginary parts as two real columns; then re = (zr qr - zi qi) + ur, im = (zr qi + zi qr) + ui;
 *   then the engine's real LU of J_k (first-maximum pivoting, zero multipliers skipped) on all 2 Fc columns at once.
 *   With r_K the result from p_0 = 0, the periodic start solves the complex system (I - z_K W_K) p_0 = r_K, W_K the
 *   periodic steady state's sensitivity of this orbit, entries ((i == j ? 1 : 0) - zKr w) + j (0 - zKi w), by the
 *   complex LU of "AC analysis"; the recursion is run again from that p_0.
 * Sidebands, m = -n_side .. n_side: P_m[q] = (1/K) sum_{k=1..K} p_k[q] (c[j] - j s[j]), j = ((m k) mod K + K) mod K:
 *   re += pr c + pi s, im += pi c - pr s, k ascending, products and sums rounded separately; the scale 1/K (one
 *   division) multiplies the finished sums.
 * Meaning: with a e^{j 2 pi f t} on the source the response on the time grid is sum_m a P_m e^{j 2 pi (f + m f0) t}: P_m
 *   at the output is the conversion gain to sideband m.  A linear circuit has P_0 = (J - z Hm)^-1 u, the AC solution
 *   with j w replaced by (1 - e^{-j w h}) / h, and P_m = 0 for m != 0.
 * Status: CSIM_ST_PAC_SINGULAR: a tiny pivot in I - z_K W_K or in a step's solve; the instance stops and its outputs
 *   for that chunk of frequencies are zeros.  An instance whose start vector or orbit is not finite gets
 *   CSIM_ST_TRAN_NONFINITE and zeros and disturbs no other; so does one that arrives with CSIM_ST_TRAN_NONFINITE or
 *   CSIM_ST_PSS_SINGULAR in d_status (what the steady state leaves of an instance it gave up), zeros without a new bit.
 *   The transient's other bits are OR-ed in as the periodic steady state does.  The device form does not check that x0
 *   closes the period: x0 is the caller's, normally csim_pss_batch_dev's.
 * Refused before anything looks at the device: null pointers, B <= 0, F <= 0 without a card, n_side < 0, numbers that
 *   are not finite, a frequency <= 0, a probe equation out of range: CSIM_ERR_ARG; no f0 / tstep and no cards, K refused
 *   as by csim_pss_num_steps, K < 2 n_side + 1, no source with an AC magnitude, sums that do not fit the LDS at one
 *   frequency per launch: CSIM_ERR_CONFIG; more than 63 unknowns: CSIM_ERR_UNSUPPORTED.
 * Card: `.PAC DEC|OCT|LIN n fstart fstop [nside]`, the grid of csim_ac_freqs, nside defaults to 1.  Any other token
 *   count, or a number that does not parse, is a card error: reported, and the card is left off.
 * csim_pac_batch_dev: freqs host [F] in Hz; probe_eq host [n_probe] or NULL = every unknown; d_x0 [N][B], not
 *   modified; d_out [F][2 n_side + 1][n_probe][B] complex, sideband m at index m + n_side; d_status [B], OR-ed.
 *   Frequencies go in chunks of the largest Fc <= 32 whose sums fit 160 KB of LDS, instances in the chunks of the
 *   periodic steady state (option pss_chunk); per instance chunk one launch for W_K, per frequency chunk two period
 *   passes around the closure solve.  LIKE csim_pss_batch_dev THIS ENTRY WAITS ON THE STREAM before it returns.
 * csim_pac_batch: DC operating point, periodic steady state (engine options pss_tol, pss_max_rounds), then the
 *   analysis; their status bits are OR-ed in.  params [B][P] or NULL (nominal); tstep <= 0: the .TRAN card's step;
 *   f0 <= 0: the .HB card's f0; freqs NULL and F == 0: the .PAC card's grid (n_side is always the caller's;
 *   csim_netlist_pac reports the card's); out [B][F][2 n_side + 1][n_probe] complex; x0_out [B][N], rounds [B],
 *   status [B] or NULL.  The exact order of every operation the analysis adds: engine/pac.hpp. */
int  csim_netlist_pac(const csim_netlist* nl, int32_t* enabled, int32_t* sweep, int32_t* n_points, double* fstart,
                      double* fstop, int32_t* n_side);
int  csim_pac_batch_dev(csim_engine* eng, const double* d_params /*[P][B]*/, int32_t B, double tstep, double f0,
                        const double* d_x0 /*[N][B]*/, const double* freqs /*host [F]*/, int32_t F, int32_t n_side,
                        const int32_t* probe_eq /*host*/, int32_t n_probe, double* d_out, uint32_t* d_status, void* stream);
int  csim_pac_batch(csim_engine* eng, const double* params, int32_t B, double tstep, double f0, const double* freqs,
                    int32_t F, int32_t n_side, const int32_t* probe_eq, int32_t n_probe, double* out, double* x0_out,
                    int32_t* rounds, uint32_t* status);

/* ---- Periodic noise analysis (.PNOISE): the adjoint of the periodic AC recursion, run backwards over the orbit ----
 * The noise at an output frequency f of a circuit on a periodic orbit is folded down from every f + m f0: each white
 * generator is modulated by the orbit and translated by it.  "Noise analysis" linearises at a DC point and cannot see
 * either.  This one solves the adjoint of "Periodic AC analysis": one column per OUTPUT frequency gives the transfer
 * from every node at every time step to the output, which serves all generators and all sidebands at once.
 * Carried over from the periodic AC analysis: h, f0, K, the table c[j], s[j], the orbit x_1 .. x_K from the given x0
 *   (integrated by the general transient's device functions in the periodic steady state's order and stored), J_k at
 *   the converged x_k, Hm, W_K, and for an output frequency f > 0 the constants z and z_K.
 * Output selector: d, real [N], +1 at out_p, -1 at out_m (-1 = ground), as in "Noise analysis".
 * Adjoint recursion, k = K down to 1, g periodic (g_0 = g_K):
 *     J_k^T q_k = z g_k + d,   g_{k-1} = Hm^T q_k.
 *   Operation order: re = (zr gr - zi gi) + d, im = (zr gi + zi gr) + 0.0; then the engine's real LU applied to the
 *   matrix J_k^T (pivots chosen on the transposed matrix, first maximum, zero multipliers skipped) on all 2 Fc real
 *   columns at once; then row i of the product over the non-zero Hm(l, i), l ascending, product and sum rounded
 *   separately.  With r = g_0 obtained from g_K = 0 the periodic start solves (I - z_K W_K^T) g_K = r, entries
 *   ((i == j ? 1 : 0) - zKr W_K(j, i)) + j (0 - zKi W_K(j, i)), by the complex LU of "AC analysis"; the recursion is run
 *   again from that g_K.
 * Generators: csim_netlist_noise_source's, in element order, evaluated at the state x_k of each step:
 *   psd_{s,k} = kT4 (1 / R) for a resistor (constant; R == 0 gives 0), kT4 ((2/3) |gg(x_k)|) for a MOSFET channel, gg
 *   from the MOSFET evaluation that assembled J_k; sigma_{s,k} = sqrt(psd_{s,k}); kT4 = 4 k_B temp_k.
 * Transfers, m = -n_side .. n_side:
 *     T_{s,m} = (1/K) sum_k sigma_{s,k} (q_k[a] - q_k[b]) (c[j] + j s[j]),  j = ((m k) mod K + K) mod K  (PLUS sign):
 *   the transfer of a unit white source at f + m f0, modulated by the orbit, to the output at f.  Per step
 *   w = sigma (q[a] - q[b]), re and im one product each; re += wr c - wi s, im += wi c + wr s.  THE STEPS ARE ADDED IN THE
 *   ORDER THE RECURSION VISITS THEM, k = K, K - 1, .. 1.  Everything is rounded separately; the scale 1/K (one division)
 *   multiplies the finished sums.
 * Outputs per (frequency, instance), |T|^2 = re re + im im:
 *   contrib[s] = 0.0 + sum_m |T_{s,m}|^2, m ascending;  side[m] = 0.0 + sum_s |T_{s,m}|^2, s ascending;
 *   onoise = 0.0 + sum_s contrib[s], s ascending, in V^2/Hz.
 * Periodic transfer function (src_elem >= 0): the same sums with sigma = 1 and the source's unit excitation in place of
 *   (a, b): a V source with branch equation k gives q_k[k], an I source (p, m) gives q_k[m] - q_k[p].  gain[m] is the
 *   conversion gain from f + m f0 at that source to the output at f; it equals the periodic AC analysis' P_{-m} at the
 *   output for the input frequency f + m f0.  Without a source a gain buffer receives zeros.
 * Status: a tiny pivot in the closure or in a step's solve sets CSIM_ST_PAC_SINGULAR (the closure matrix is the
 *   periodic AC analysis' transposed: the same condition); the instance's outputs for that chunk of frequencies are
 *   +0.0.  A start that is not finite, and instances that arrive with CSIM_ST_TRAN_NONFINITE or CSIM_ST_PSS_SINGULAR,
 *   behave as in the periodic AC analysis.
 * Refused before anything looks at the device: what the periodic AC analysis and the noise analysis refuse -- null
 *   pointers, B <= 0, F <= 0 without a card, n_side < 0, numbers that are not finite, a frequency <= 0, out_p == out_m
 *   or out_p < 0 or an equation out of range, a src_elem that is not a V or I source: CSIM_ERR_ARG; temp_k <= 0 or not
 *   finite, no f0 / tstep and no cards, K refused as by csim_pss_num_steps, K < 2 n_side + 1, sums that do not fit the
 *   LDS at one frequency per launch, an orbit of one instance (K N 8 bytes) beyond the orbit store's budget:
 *   CSIM_ERR_CONFIG; more than 63 unknowns: CSIM_ERR_UNSUPPORTED.  No AC source is needed.
 * Card: `.PNOISE V(out[,ref]) [src] DEC|OCT|LIN n fstart fstop [nside]`: output and source as .NOISE's, grid and nside
 *   (default 1) as .PAC's.  A card error is reported and the card left off.
 * csim_pnoise_batch_dev: freqs host [F] in Hz; d_x0 [N][B], not modified; d_onoise [F][B]; d_gain
 *   [F][2 n_side + 1][B] complex or NULL; d_contrib [F][S][B] or NULL; d_side [F][2 n_side + 1][B] or NULL, sideband m
 *   at index m + n_side; d_status [B], OR-ed.  Frequencies go in chunks of the largest Fc <= 32 whose LDS image (the
 *   general kernel's, Hm, the g and q planes, the generators' sigma and equations, 2 (S + 1)(2 n_side + 1) Fc sums)
 *   fits 160 KB; instances in the chunks of the periodic steady state (option pss_chunk), reduced so that the orbit
 *   store, chunk K N 8 bytes, stays within 256 MiB.  Per instance chunk one launch for W_K and one for the orbit, per
 *   frequency chunk two backward passes around the closure solve.  THIS ENTRY WAITS ON THE STREAM before it returns.
 * csim_pnoise_batch: DC operating point, periodic steady state, then the analysis; their status bits are OR-ed in.
 *   params [B][P] or NULL (nominal); tstep <= 0: the .TRAN card's step; f0 <= 0: the .HB card's f0; freqs NULL and
 *   F == 0: the .PNOISE card's grid; out_p_eq == -2: the card's output and source (n_side is always the caller's;
 *   csim_netlist_pnoise reports the card's); onoise [B][F], gain [B][F][2 n_side + 1] complex, contrib [B][F][S],
 *   side [B][F][2 n_side + 1], x0_out [B][N], rounds [B], status [B]; all but onoise may be NULL.
 *   The exact order of every operation the analysis adds: engine/pnoise.hpp. */
int  csim_netlist_pnoise(const csim_netlist* nl, int32_t* enabled, int32_t* out_p_eq, int32_t* out_m_eq, int32_t* src_elem,
                         int32_t* sweep, int32_t* n_points, double* fstart, double* fstop, int32_t* n_side);
int  csim_pnoise_batch_dev(csim_engine* eng, const double* d_params /*[P][B]*/, int32_t B, double tstep, double f0,
                           const double* d_x0 /*[N][B]*/, const double* freqs /*host [F]*/, int32_t F, int32_t n_side,
                           int32_t out_p_eq, int32_t out_m_eq, int32_t src_elem, double temp_k, double* d_onoise,
                           double* d_gain, double* d_contrib, double* d_side, uint32_t* d_status, void* stream);
int  csim_pnoise_batch(csim_engine* eng, const double* params, int32_t B, double tstep, double f0, const double* freqs,
                       int32_t F, int32_t n_side, int32_t out_p_eq, int32_t out_m_eq, int32_t src_elem, double temp_k,
                       double* onoise, double* gain, double* contrib, double* side, double* x0_out, int32_t* rounds,
                       uint32_t* status);

/* Batched dense solve A x = b with the engine's pivoted LU
 * (Solver::solveLinearSystemLU semantics: first-maximum partial pivoting,
 * tiny pivot -> zero vector).  A [B][n][n] row-major, b/x [B][n], host
 * pointers.  flags [B] optional (CSIM_ST_LU_*).  device: HIP device index.
 * n <= 63 runs LDS-resident, 64 <= n <= 1024 in place in global memory.       */
int  csim_lu_solve_batch(int32_t device, int32_t n, int32_t B, const double* A,
                         const double* b, double* x, uint32_t* flags);
/* The complex counterpart: B systems (G + j w C) x = J at F angular frequencies through the AC sweep kernels of
 * "AC analysis" above (same pivot rule, multiplier, order; lu_eps = 1e-15), without an engine or a netlist.
 * Host pointers.  G, C [B][n][n] row-major; J [B][n] complex (re, im) pairs; omega [F] rad/s, used as given;
 * x [B][F][n] complex pairs (the zero vector where the factorisation fails); flags [B] optional (CSIM_ST_LU_*).
 * kernel: 0 auto (packed for n <= 32), 1 wave (n <= 63), 2 packed (n <= 32), 4 block (n <= 1024; never picked by
 * auto; AC and noise only: csim_sp_solve_batch and csim_spnoise_solve_batch answer it with CSIM_ERR_UNSUPPORTED);
 * any other value, 3 included: CSIM_ERR_ARG; a size beyond the kernel: CSIM_ERR_UNSUPPORTED.  n, B or F == 0:
 * nothing to do.                                                                                                */
int  csim_ac_solve_batch(int32_t device, int32_t n, int32_t B, const double* G, const double* C,
                         const double* J, const double* omega, int32_t F, int32_t kernel,
                         double* x, uint32_t* flags);

/* The noise kernels on systems and generator tables given directly (host pointers; lu_eps = 1e-15), the counterpart
 * of csim_ac_solve_batch for "Noise analysis".  G, C [B][n][n] row-major; generators src_a, src_b [S] (equations, -1
 * ground) with psd [B][S]; in_kind 0: no gain, 1: H = y[in_a], 2: H = y[in_a] - y[in_b] (-1 ground); omega [F] rad/s.
 * onoise [B][F]; contrib [B][F][S], gain [B][F] complex, y [B][F][n] complex (the adjoint solution, zeros where
 * the factorisation fails) and flags [B] are optional.  kernel and sizes as csim_ac_solve_batch; an equation index
 * out of range: CSIM_ERR_ARG.                                                                                     */
int  csim_noise_solve_batch(int32_t device, int32_t n, int32_t B, const double* G, const double* C, int32_t out_p,
                            int32_t out_m, int32_t S, const int32_t* src_a, const int32_t* src_b, const double* psd,
                            int32_t in_kind, int32_t in_a, int32_t in_b, const double* omega, int32_t F,
                            int32_t kernel, double* onoise, double* contrib, double* gain, double* y, uint32_t* flags);

/* The S-parameter kernels on systems given directly (host pointers; lu_eps = 1e-15), the counterpart of
 * csim_ac_solve_batch for "S-parameter analysis".  G, C [B][n][n] row-major; omega [F] rad/s; 1 <= K <= 4.
 *   port_eq == NULL: K right-hand sides J [B][K][n] complex, solutions x [B][F][K][n] complex.
 *   port_eq [K], z0 [K]: the right-hand sides are the unit vectors at port_eq (J is not read); y [B][F][K][K] complex,
 *   s the same or NULL, x optional.
 * flags [B] optional.  kernel and sizes as csim_ac_solve_batch; K outside 1 .. 4, an equation out of range or a Z0
 * that is not finite and > 0: CSIM_ERR_ARG.                                                                        */
int  csim_sp_solve_batch(int32_t device, int32_t n, int32_t B, int32_t K, const double* G, const double* C,
                         const double* J, const double* omega, int32_t F, int32_t kernel, double* x, uint32_t* flags,
                         const int32_t* port_eq, const double* z0, double* y, double* s);

/* The two-port noise kernels on systems, ports and generator tables given directly (host pointers; lu_eps = 1e-15),
 * the counterpart of csim_ac_solve_batch for "Two-port noise analysis".  G, C [B][n][n] row-major; port_eq [P],
 * z0 [P] (Gs = 1 / z0[0]), 1 <= P <= 4; generators src_a, src_b [S] (equations, -1 ground) with psd [B][S]; omega [F]
 * rad/s.  cy [B][F][P][P] complex; y the same, nf, fmin, rn [B][F], yopt [B][F] complex, x [B][F][P][n] complex (the
 * adjoint solutions, zeros where the factorisation fails) and flags [B] are optional.  kernel and sizes as
 * csim_ac_solve_batch; P outside 1 .. 4, an equation index out of range or a Z0 that is not finite and > 0:
 * CSIM_ERR_ARG; a noise parameter asked for with P != 2: CSIM_ERR_CONFIG.                                          */
int  csim_spnoise_solve_batch(int32_t device, int32_t n, int32_t B, int32_t P, const double* G, const double* C,
                              const int32_t* port_eq, const double* z0, int32_t S, const int32_t* src_a,
                              const int32_t* src_b, const double* psd, const double* omega, int32_t F, int32_t kernel,
                              double* y, double* cy, double* nf, double* fmin, double* rn, double* yopt, double* x,
                              uint32_t* flags);

/* The distortion kernels on systems and device tables given directly (host pointers; lu_eps = 1e-15), the counterpart
 * of csim_ac_solve_batch for "Distortion analysis".  G, C [B][n][n] row-major; J [B][n] complex (re, im) pairs; devices
 * dev_d, dev_g, dev_s [M] (equations, -1 ground) with coef [B][M][7] in the order of that section; omega [F] rad/s.
 * hd [B][F][2]; h [B][F][3][n] complex (zeros from the failed order on) and flags [B] are optional.  kernel 0 auto
 * (packed for n <= 32), 1 wave (n <= 63), 2 packed (n <= 32); 4 (block): CSIM_ERR_UNSUPPORTED; any other value, 3
 * included: CSIM_ERR_ARG; an equation index out of range, or out_p == out_m: CSIM_ERR_ARG.                        */
int  csim_disto_solve_batch(int32_t device, int32_t n, int32_t B, const double* G, const double* C, const double* J,
                            int32_t M, const int32_t* dev_d, const int32_t* dev_g, const int32_t* dev_s,
                            const double* coef, int32_t out_p, int32_t out_m, const double* omega, int32_t F,
                            int32_t kernel, double* h, double* hd, uint32_t* flags);

/* The intermodulation kernels on systems and device tables given directly (host pointers; lu_eps = 1e-15), the
 * counterpart of csim_disto_solve_batch for "Intermodulation analysis".  J [B][n] complex excites the first tone, J2 the
 * second (NULL: J); omega1, omega2 [F] rad/s, any finite values (else CSIM_ERR_ARG).  im [B][F][3]; h [B][F][6][n]
 * complex (zeros from the failed solve on) and flags [B] are optional.  Kernels and refusals as csim_disto_solve_batch. */
int  csim_imd_solve_batch(int32_t device, int32_t n, int32_t B, const double* G, const double* C, const double* J,
                          const double* J2, int32_t M, const int32_t* dev_d, const int32_t* dev_g, const int32_t* dev_s,
                          const double* coef, int32_t out_p, int32_t out_m, const double* omega1, const double* omega2,
                          int32_t F, int32_t kernel, double* h, double* im, uint32_t* flags);

/* The loop-gain kernels on systems given directly (host pointers; lu_eps = 1e-15), the counterpart of
 * csim_ac_solve_batch for "Loop-gain analysis".  G, C [B][n][n] row-major; eq_p, eq_m, eq_br the probe's + node, - node
 * and branch equations, three different values in 0 .. n-1 (else CSIM_ERR_ARG); omega [F] rad/s.  T [B][F] complex;
 * x [B][F][2][n] complex and flags [B] are optional.  margins [B][4] (optional) needs freqs_hz [F], strictly increasing
 * and positive (else CSIM_ERR_ARG); found [B] int32 (optional) needs margins.  kernel 0 auto (packed for n <= 32), 1 wave
 * (n <= 63), 2 packed (n <= 32); 4 (block): CSIM_ERR_UNSUPPORTED; any other value, 3 included: CSIM_ERR_ARG.  Nothing
 * is written when n, B or F is 0.                                                                                   */
int  csim_stb_solve_batch(int32_t device, int32_t n, int32_t B, const double* G, const double* C, int32_t eq_p, int32_t eq_m,
                          int32_t eq_br, const double* omega, int32_t F, int32_t kernel, double* T, double* x,
                          uint32_t* flags, const double* freqs_hz, double* margins, int32_t* found);

/* The pole kernel on systems given directly (host pointers; lu_eps = 1e-15), "Pole analysis" on any (G, C).  G, C
 * [B][n][n] row-major.  poles [B][n] complex; n_poles, n_rhp [B] int32, max_re [B] and flags [B] (CSIM_ST_PZ_*) are
 * optional.  fmax not finite or <= 0, sigma0 not finite: CSIM_ERR_ARG; then n > 63: CSIM_ERR_UNSUPPORTED.  Nothing is
 * written when n or B is 0.                                                                                         */
int  csim_pz_solve_batch(int32_t device, int32_t n, int32_t B, const double* G, const double* C, double fmax, double sigma0,
                         double* poles, int32_t* n_poles, int32_t* n_rhp, double* max_re, uint32_t* flags);

/* ---- Gauss-Seidel variant of the reference (never reached from its main(), kept as public API) ----
 * Batched Solver::solveLinearSystemGaussSeidel (include/solver.hpp:139-204): sweeps in row order with the
 * newest values, a diagonal below 1e-12 replaced by +-1e-12, stop when ||x - x_prev|| < tol or after
 * max_iters sweeps; whatever the sweeps left is returned (it may be non-finite).  A [B][n][n] row-major,
 * b / x0 / x [B][n] host pointers; x0 NULL = start from zero (the two-argument overload); sweeps [B]
 * optional = sweeps performed.  One lane per system, same operation order as the reference.            */
int  csim_gs_solve_batch(int32_t device, int32_t n, int32_t B, const double* A, const double* b,
                         const double* x0, int32_t max_iters, double tol, double* x, int32_t* sweeps);
/* dcSolveGaussSeidel (src/dcanalysis.cpp:71-92,166-237,254-258) for B instances: linear circuits one
 * Gauss-Seidel solve (2000 sweeps, 1e-10), circuits with MOSFETs the source ramp with 60 (last step 120)
 * Newton passes per step, inner solve warm-started from x, ConvController update.  A pass whose inner
 * solve turns non-finite raises gmin x10 and is dropped (CSIM_ST_DC_NONFINITE), exactly as upstream; on
 * circuits with voltage sources (zero diagonal entries) that is every pass and x stays 0.  A LINEAR
 * circuit whose sweeps diverge returns what the reference's dense loops leave (a pattern of +-inf / NaN,
 * reproduced component by component) and no flag -- upstream checks nothing there (:89-91).  N <= 63.   */
int  csim_dc_gs_batch_dev(csim_engine* eng, const double* d_params /*[P][B]*/, int32_t B,
                          double* d_x /*[N][B]*/, int32_t* d_iters, uint32_t* d_status, void* stream);
int  csim_dc_gs_batch(csim_engine* eng, const double* params /*[B][P] or NULL*/, int32_t B,
                      double* x_out /*[B][N]*/, int32_t* nr_iters, uint32_t* status);

/* Runtime specialisation for a netlist without a prebuilt libcsim_sched_<topology>.so:
 * records the pivot schedule of instance 0 of d_params with the general kernel
 * (plan_steps transient steps), generates the lane-per-instance kernel, compiles it
 * (up to 4 distinct sequences seen while planning become alternatives), compiles it
 * with hipcc (--offload-arch=gfx950; a child process started from an argument vector,
 * no shell, killed after jit_timeout seconds) into the private JIT cache directory
 * (csim_engine_set_option) and loads it.  A cached library is reused only if it is the
 * caller's own regular file and reports the hash of exactly this (topology, constants,
 * schedules, generator revision).  After CSIM_OK, csim_engine_tran_kernel() reports
 * "scheduled".                                                                      */
int  csim_engine_jit_scheduled(csim_engine* eng, const double* d_params /*[P][B]*/, int32_t B,
                               double tstep, int64_t plan_steps);
/* The build half of the above for schedules the caller already has (from the planner
 * entry points below, or from a schedule file): pivot_pos [n_alts][N] transient
 * sequences, most frequent first (1..16); dc_pivot_pos [n_dc_alts][N] sequences of the DC
 * operating point (0..8; 0 = no DC kernel).  Schedules decide speed only: every
 * factorisation re-verifies the sequence it uses.                                   */
int  csim_engine_jit_with_schedules(csim_engine* eng, const int32_t* pivot_pos, int32_t n_alts,
                                    const int32_t* dc_pivot_pos, int32_t n_dc_alts);

/* Batched Solver::luDecompose (include/solver.hpp:30-80): LU [B][n][n] holds U on
 * and above the diagonal and the multipliers below it, perm [B][n] the row
 * permutation (b_perm[i] = b[perm[i]]).  flags[b] = CSIM_ST_LU_TINY_PIVOT where
 * the reference returns false (LU/perm of that system are then unspecified).  */
int  csim_lu_decompose_batch(int32_t device, int32_t n, int32_t B, const double* A,
                             double* LU, int32_t* perm, uint32_t* flags);

/* Planner: run DC + n_steps transient steps of ONE instance (column `instance` of
 * d_params) with the general kernel and report the partial-pivot row position chosen
 * for every column in the first transient factorisation (pivot_pos[N], host), the
 * number of factorisations seen and how many used a different sequence.  This is what
 * a schedule file of csrc/schedules/ is recorded from.                              */
int  csim_record_pivot_schedule(csim_engine* eng, const double* d_params /*[P][B]*/, int32_t B,
                                int32_t instance, double tstep, int64_t n_steps,
                                int32_t* pivot_pos, int64_t* n_factorizations, int64_t* n_differ);
/* Same run, every DISTINCT sequence seen (at most 8, most frequent first): pivot_pos
 * [max_alts][N], counts [max_alts] = factorisations that used each, *n_alts = how many were
 * found, *n_other = factorisations that failed or used a sequence beyond the eighth.  A
 * switching circuit alternates between a few sequences; a schedule file may list several. */
int  csim_record_pivot_schedules(csim_engine* eng, const double* d_params /*[P][B]*/, int32_t B,
                                 int32_t instance, double tstep, int64_t n_steps, int32_t max_alts,
                                 int32_t* pivot_pos, int64_t* counts, int32_t* n_alts, int64_t* n_other);
/* The same planner on the DC operating point of instance `instance` (source ramp + adaptive
 * gmin, reference src/dcanalysis.cpp:95-163): its distinct pivot sequences, most frequent first
 * ("dc" lines of a schedule file).  Circuits of up to 63 unknowns.                           */
int  csim_record_dc_pivot_schedules(csim_engine* eng, const double* d_params /*[P][B]*/, int32_t B,
                                    int32_t instance, int32_t max_alts, int32_t* pivot_pos,
                                    int64_t* counts, int32_t* n_alts, int64_t* n_other);

#ifdef __cplusplus
}
#endif
#endif /* CSIM_H */
