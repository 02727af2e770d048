/*
 * smrt_dort.h -- C ABI of the MI355X-native DORT hot path (libsmrt_dort.so).
 *
 * The reference (smrt-model/smrt) is pure Python and has no FFI; the interface these entry points replace is the
 * reference's plugin surface for this path (all paths relative to /root/reference):
 *
 *   smrt_dort_run()      <->  one call of runner(function, argument_list)        smrt/core/model.py:395-398
 *                             = for every (sensor_f, snowpack): Model.run_single_simulation
 *                                                                                smrt/core/model.py:584-619
 *                             = prepare_emmodels (IBA / DMRT_QCA_ShortRange ctor) smrt/core/model.py:529-582,
 *                               smrt/emmodel/iba.py:85-137, smrt/emmodel/dmrt_qca_shortrange.py:65-112
 *                             + DORT.solve                                       smrt/rtsolver/dort.py:189-261
 *   smrt_batch           <->  the flattened (frequency-major) simulation list    smrt/core/model.py:476-527
 *                             and the DORT constructor options                   smrt/rtsolver/dort.py:148-178
 *   status[]             <->  SMRTError / error_handling="nan"                   smrt/rtsolver/dort.py:327-334
 *   layer_out/stream_out <->  Result.other_data                                  smrt/rtsolver/rtsolver_utils.py:338-342,373-398
 *
 * Plain C types only: the caller owns every host buffer (C-contiguous float64 / int32); the library owns the
 * device memory inside the context.  One context per GPU, one host thread per context, no global state.
 */
#ifndef SMRT_DORT_H
#define SMRT_DORT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* The library is built with -fvisibility=hidden: exactly the entry points declared here are exported. */
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

typedef struct smrt_dort_ctx smrt_dort_ctx;

/* emmodel (smrt/emmodel/iba.py, dmrt_qca_shortrange.py, dmrt_qcacp_shortrange.py, nonscattering.py) */
#define SMRT_EM_IBA 0
#define SMRT_EM_DMRT_QCA_SHORTRANGE 1
#define SMRT_EM_DMRT_QCACP_SHORTRANGE 2
#define SMRT_EM_NONSCATTERING 3
#define SMRT_EM_HOST 4   /* any other emmodel, evaluated by the caller: see smrt_batch.host_layer / host_phase */
/* IBA with dense_snow_correction="auto" on a layer of more than half ice (smrt/emmodel/iba.py:95-96 ->
 * smrt/core/layer.py:186-201): air inclusions in an ice background.  The layer's frac_volume entry is then the volume
 * fraction of the INCLUSIONS, i.e. 1 - (ice fraction), exactly what the reference's inverted layer carries. */
#define SMRT_EM_IBA_INVERTED 5
/* IBA's PHASE FUNCTION on the layer's microstructure model with the layer's SCALARS from the caller: every emmodel whose
 * phase matrix is (coefficient) x (Fourier transform of the autocorrelation function at 2 k0 Re sqrt(eps_eff) sin(Theta/2)) x
 * (Rayleigh geometry) -- smrt/emmodel/iba.py:228-244 -- and that differs from IBA in the numbers only: iba_original.py
 * (absorption), iba_maxwell_garnett.py (mixing formula, field ratio), derived_IBA(<mixing formula>), IBA on layers with
 * another permittivity model, non-spherical inclusions, a background that is not air (saline ice).  host_layer holds
 * (ks, ka, Re eps_eff, Im eps_eff) of the layer as for SMRT_EM_HOST, host_iba_coeff the coefficient (iba.py:139-150);
 * frac_volume and micro_p1 / micro_p2 are the ones of the (possibly inverted) medium the emmodel works on.  The phase
 * matrices are assembled on the device: no host_streams / host_phase. */
#define SMRT_EM_IBA_HOST 6
/* The RAYLEIGH phase matrix, 3 ks / 2 x the geometry of smrt/emmodel/rayleigh.py:52-127, with the layer's scalars from the
 * caller (host_layer = ks, ka, Re eps_eff, Im eps_eff): every emmodel that inherits ft_even_phase from smrt's Rayleigh --
 * rayleigh.py, sft_rayleigh.py, prescribed_kskaeps.py, the dmrt short-range emmodels on layers the device versions
 * refuse.  The microstructure code and parameters of such a layer are not read. */
#define SMRT_EM_RAYLEIGH_HOST 7
/* microstructure (smrt/microstructure_model/exponential.py, sticky_hard_spheres.py) */
#define SMRT_MS_EXPONENTIAL 0
#define SMRT_MS_STICKY_HARD_SPHERES 1   /* micro_p1 = radius, micro_p2 = stickiness (> 0), or -t: the parameter t itself
                                        * (unified_sticky_hard_spheres.py:24-27; IBA only -- the dmrt emmodels take a stickiness) */
#define SMRT_MS_INDEPENDENT_SPHERE 2   /* micro_p1 = radius (smrt/microstructure_model/independent_sphere.py:54-72); IBA only */
#define SMRT_MS_TEUBNER_STREY 3        /* micro_p1 = corr_length xi, micro_p2 = Y = (2 pi xi / repeat_distance)^2 (teubner_strey.py:45-55); a
                                        * negative Y gives the two-length form of unified_teubner_strey.py:69-72; IBA only */
/* The exponential model evaluated at the COMPLEX wavenumber of the strong-contrast-expansion emmodels (smrt/emmodel/
 * sce_common.py:222-233: 2 k0 sqrt(eps_eff) sin(Theta / 2) with the complex eps_eff, real part of the transform kept,
 * emmodel/common.py:107-117): micro_p1 = corr_length; eps_eff comes from host_layer.  Only as the microstructure code of
 * SMRT_EM_IBA_HOST layers (layer_kind), passive mode.  Teubner-Strey's expression likewise (4 + its own code, micro_p1 /
 * micro_p2 as for SMRT_MS_TEUBNER_STREY).  The codes of the sphere models are reserved and refused: their complex form
 * (sines of the complex k r) cost the headline pipeline's prep kernel more than it was worth; such layers take the
 * SMRT_EM_HOST route. */
#define SMRT_MS_EXPONENTIAL_COMPLEX_K 4
#define SMRT_MS_STICKY_HARD_SPHERES_COMPLEX_K 5
#define SMRT_MS_INDEPENDENT_SPHERE_COMPLEX_K 6
#define SMRT_MS_TEUBNER_STREY_COMPLEX_K 7
/* sensor mode (smrt/core/sensor.py:330-339) */
#define SMRT_MODE_PASSIVE 0
#define SMRT_MODE_ACTIVE 1
/* DORT phase_normalization (smrt/rtsolver/dort.py:94-103): False / "auto"|True / "forced" */
#define SMRT_NORM_OFF 0
#define SMRT_NORM_ON 1
#define SMRT_NORM_FORCED 2

/* substrate under the last layer */
#define SMRT_SUBSTRATE_NONE 0       /* semi-infinite / transparent (rtsolver_utils.py:548-551,601-603) */
#define SMRT_SUBSTRATE_FLAT 1       /* Fresnel against a given permittivity (substrate/flat.py) */
#define SMRT_SUBSTRATE_REFLECTOR 2  /* prescribed specular reflection, emissivity 1 - R (substrate/reflector.py), passive only */
#define SMRT_SUBSTRATE_HOST 3       /* rough substrate: dense reflection matrices (+ emissivity in passive mode) evaluated by the caller */
/* Rough soils, passive mode only: Fresnel against the soil permittivity times a roughness factor per polarisation, evaluated
 * per stream on the device; emissivity 1 - R.  Their parameters follow the permittivities in substrate_p1 / substrate_p2. */
#define SMRT_SUBSTRATE_SOIL_WEGMULLER 4   /* Wegmuller & Maetzler 1999 (substrate/soil_wegmuller.py): roughness_rms */
#define SMRT_SUBSTRATE_SOIL_QNH 5         /* Wang 1983 (substrate/soil_qnh.py): H, Q, Nv, Nh */
#define SMRT_SUBSTRATE_ROUGH_CHOUDHURY 6  /* Choudhury et al. 1979 (substrate/rough_choudhury79.py): roughness_rms; a pair with
                                           * ksigma > 0.1 in its last layer gets the status SMRT_ERR_INPUT */

/* per-pair status word */
#define SMRT_OK 0
#define SMRT_ERR_EIGEN 1           /* eigen iteration did not converge (dort.py:1068-1085)                */
#define SMRT_ERR_NORMALIZATION 2   /* phase renormalisation beyond 30 % (dort.py:792-801)                 */
#define SMRT_ERR_ALBEDO 3          /* single scattering albedo >= 1: no real eigenvalues (dort.py:941)    */
#define SMRT_ERR_SINGULAR 4        /* singular boundary-condition system                                  */
#define SMRT_ERR_INPUT 5           /* invalid layer input (e.g. T > 273.15 K, ice.py:56-57; < 2 streams)   */
#define SMRT_ERR_COHERENT 6        /* process_coherent_layers: the last layer, or two layers in a row, are coherent (coherent_flat.py:26,34) */

/*
 * A batch = S snowpacks x F frequencies, flattened frequency-major exactly like Model.prepare_simulations
 * (pair p = f * S + s).  Per-layer arrays are row-major [S][n_layers_max], layer 0 at the top.
 */
typedef struct smrt_batch {
    int32_t n_snowpacks;      /* S */
    int32_t n_layers_max;     /* row length of the per-layer arrays */
    int32_t n_frequencies;    /* F */
    int32_t n_theta;          /* number of viewing angles (passive) or incidence angles (active) */
    int32_t emmodel;          /* SMRT_EM_* */
    int32_t microstructure;   /* SMRT_MS_* */
    int32_t mode;             /* SMRT_MODE_* */
    int32_t n_max_stream;     /* DORT n_max_stream (dort.py:150) */
    int32_t m_max;            /* DORT m_max, used in active mode only (dort.py:151,209) */
    int32_t phase_normalization; /* SMRT_NORM_* */
    int32_t rayleigh_jeans;   /* DORT rayleigh_jeans_approximation (dort.py:160) */
    int32_t substrate_kind;   /* SMRT_SUBSTRATE_*: what lies under the last layer (Snowpack.substrate) */
    const int32_t* n_layers;  /* [S] */
    const double* thickness;  /* [S][Lmax] m */
    const double* frac_volume;/* [S][Lmax] ice volume fraction (SnowLayer.compute_frac_volumes, make_medium.py:390-434) */
    const double* temperature;/* [S][Lmax] K */
    const double* micro_p1;   /* [S][Lmax] corr_length (exponential) | radius (sticky_hard_spheres), m */
    const double* micro_p2;   /* [S][Lmax] unused (exponential, independent_sphere) | stickiness or -t (sticky_hard_spheres) |
                               * Y (teubner_strey): see SMRT_MS_* */
    const double* frequency;  /* [F] Hz */
    const double* theta;      /* [n_theta] rad: Sensor.theta (== theta_inc in active/backscatter mode) */
    double phi;               /* active: azimuth (rad), pi for backscatter (sensor.py:179-180) */
    /* substrate (smrt/substrate/flat.py, reflector.py; rtsolver_utils.py:544-605, dort.py:429-441), per pair because
     * permittivity / reflection models may depend on the frequency.  Unused (may be NULL) for SMRT_SUBSTRATE_NONE. */
    const double* substrate_p1;          /* [F][S] flat: Re eps_substrate | reflector: specular reflection, V
                                          * SMRT_SUBSTRATE_SOIL_WEGMULLER .. _ROUGH_CHOUDHURY: [F][S] Re eps_soil, FOLLOWED BY [S][2]:
                                          * (roughness_rms in m, unused) for Wegmuller and Choudhury, (H, Q) for QNH */
    const double* substrate_p2;          /* [F][S] flat: Im eps_substrate | reflector: specular reflection, H
                                          * the soil kinds: [F][S] Im eps_soil, FOLLOWED BY [S][2]: (Nv, Nh) for QNH, unused
                                          * (but present) for the two others */
    const double* substrate_temperature; /* [S] K; <= 0: the substrate does not emit (temperature=None) */
    /* SimpleIsotropicAtmosphere (smrt/atmosphere/simple_isotropic_atmosphere.py; rtsolver_utils.py:251-260,302-305),
     * passive mode only; all three NULL = no atmosphere */
    const double* atm_tb_down;           /* [F] K */
    const double* atm_tb_up;             /* [F] K */
    const double* atm_transmittance;     /* [F] */
    /* DORT option prune_deep_snowpack (dort.py:117-124,176-178,443-452): optical depth (sum over the layers, from the
     * top, of min|beta_l| * thickness_l) beyond which the deeper layers are left out of the solve; the layer in which
     * the threshold is passed keeps its bottom reflection and receives nothing from below.  <= 0 (or NaN): off.
     * Needs a three-kernel pipeline (the eigenvalues of all the layers are known before the boundary recursion starts;
     * every size up to the limit of 384 streams x polarisations has one): smrt_dort_upload fails only after
     * smrt_dort_set_pipeline(ctx, 0).  The prep and Jacobi kernels then run in up to four rounds over successive layer
     * ranges, so the layers below a cut are never diagonalised. */
    double prune_optical_depth;
    /* Heterogeneous snowpacks (a list / dict of emmodels in make_model, per-layer microstructure models in make_snowpack;
     * smrt/core/model.py:529-582): [S][Lmax] emmodel + 16 * microstructure of every layer (SMRT_EM_* + 16 * SMRT_MS_*).
     * NULL: every layer uses `emmodel` / `microstructure` above. */
    const int32_t* layer_kind;
    /* Electromagnetic models evaluated by the caller -- any object with the reference's emmodel protocol
     * (effective_permittivity, ks, ka, ft_even_phase; smrt/rtsolver/dort.py:189,231-247,714-762).  Layers whose kind is
     * SMRT_EM_HOST take their scalars and the azimuth modes of their phase matrix from these arrays instead of
     * evaluating an emmodel on the device; everything else (streams, interfaces, diagonalisation, boundary system) is
     * the same device path.  Indexed by the pair p = f * S + s.  All NULL when no layer is of that kind.
     *   host_layer   [F * S][Lmax][4]: ks, ka (1/m, isotropic), Re and Im of the effective permittivity
     *   host_streams [F * S][Lmax]: number of streams of the layer as the caller computed it (streams.py:136-223);
     *                the device checks it against its own count (SMRT_ERR_INPUT on a mismatch)
     *   host_phase   [F * S][Lmax][modes][2][NE * NE], modes = 1 (passive) or m_max + 1 (active), NE = n_max_stream *
     *                polarisations (2 passive, 3 active): ft_even_phase(mu, +mu') and ft_even_phase(mu, -mu') of
     *                mode m on the layer's own stream cosines, compressed like smrt/core/lib.py:336-347 (row =
     *                stream_s * polarisations + pol_s, column = stream_i * polarisations + pol_i), row-major with
     *                leading dimension NE; only the rows / columns below n_l * polarisations are read.  The matrix
     *                must obey reciprocity (symmetric P(mu,+mu'), P(mu,-mu') up to the sign / factor 2 conventions
     *                of the U polarisation, emmodel/common.py:40-50): the device reads its lower triangle. */
    const double* host_layer;
    const int32_t* host_streams;
    const double* host_phase;
    /* DORT option process_coherent_layers (dort.py:110,156,203; rtsolver_utils.py:349-365; interface/coherent_flat.py):
     * non-zero = per pair, every layer with k0 Re(sqrt(eps_eff)) thickness < 3 pi / 4 at the pair's frequency is taken
     * out of the snowpack and becomes a coherent (Fabry-Perot) interface on top of the layer below it; layer_out then
     * holds the remaining layers, top first, and zeros after them, with 1024 x (index of the layer in the input) added to
     * the stream count of column 4 so that the caller can tell which layers were kept.  With SMRT_EM_HOST layers the
     * host_* arrays stay indexed by the layer's position in the INPUT; host_streams / host_phase of a layer that stays
     * must then be sampled on the streams of the REDUCED snowpack (the caller applies the same criterion to its own
     * permittivities: the most refringent layer is searched among the layers that stay), entries of layers that leave are
     * not read apart from the permittivity. */
    int32_t process_coherent_layers;
    /* SMRT_SUBSTRATE_HOST: a rough substrate (smrt/substrate/geometrical_optics.py, iem_fung92*.py, ...).  The reflection
     * matrix of the bottom boundary is no longer diagonal; the caller evaluates it with the reference's own substrate
     * classes exactly as compute_interface_properties does (rtsolver_utils.py:567-597,690-707: specular_reflection_matrix
     * on the diagonal + 2 pi (mode 0) | pi (mode >= 1) x ft_even_diffuse_reflection_matrix normalised by mu and the
     * stream weights) on the streams of the LAST layer, and the device starts its bottom-up recursion from it.  Indexed
     * by the pair p = f * S + s; modes = m_max + 1 in active mode, 1 in passive mode; NE = 3 * n_max_stream:
     *   host_substrate     [F * S][modes][NE * NE]: reflection_bottom(last layer, mode m), compressed (row = scattered
     *                      stream * P + polarisation, column = incident; P = 2 for mode 0, 3 above), row-major with
     *                      leading dimension NE; rows / columns below n_last * P are read
     *   host_substrate_coh [F * S][modes][NE]: active mode: the diagonal of its specular part (coherent-only pass, mode
     *                      0 is used); passive mode: the emissivity diagonal (substrate.emissivity_matrix,
     *                      rtsolver_utils.py:533-536), multiplied by B(substrate_temperature[s]) on the device
     * (The reference runs its purely diffuse substrates -- geometrical_optics -- in active mode only: in passive mode it
     * raises, dort.py:437; iem_fung92*, geometrical_optics_backscatter run in both.)  Under process_coherent_layers the
     * caller samples them on the streams of the REDUCED snowpack (the layers with k0 Re(n) d >= 3 pi / 4). */
    const double* host_substrate;
    const double* host_substrate_coh;
    /* SMRT_INTERFACE_HOST: rough interfaces at the surface or between layers (smrt/interface/iem_fung92.py,
     * geometrical_optics.py, ...; smrt/rtsolver/rtsolver_utils.py:473-642).  Their reflection / transmission matrices are
     * dense in the streams; the caller evaluates them with the reference's own interface classes exactly as
     * compute_interface_properties combines them (specular / coherent part on the diagonal + 2 pi (mode 0) | pi (mode >= 1)
     * x the diffuse mode normalised by mu and the stream weights) and the device composes each of them with the
     * reflection matrix of everything below (one N x N solve and two products per rough interface and mode).
     *   host_interface_slot [F * S][n_layers_max] int32: -1 = the interface ON TOP of this layer is Flat (Fresnel on the
     *                       device); k >= 0 = it is rough and slot k of host_interface holds it (layer 0: the surface);
     *   host_interface      [F * S][host_interface_slots][modes][4][NE * NE], modes = m_max + 1 in active mode, 1 in passive
     *                       mode, NE = 3 * n_max_stream, row-major with leading dimension NE, compressed order (stream * P +
     *                       polarisation; P = 2 for mode 0, 3 above), zero outside the streams that exist:
     *                         [0] Rtop  reflection_top(layer):       rows and columns = streams of the layer
     *                         [1] Ttop  transmission_top(layer):     rows = streams of the medium above, columns = of the layer
     *                         [2] Rbot  reflection_bottom(above):    rows and columns = streams of the medium above
     *                         [3] Tbot  transmission_bottom(above):  rows = streams of the layer, columns = of the medium above
     *                       (a purely specular transmission is diagonal and is cut to the common streams, like the
     *                       reference does, dort.py:372-376,409-414);
     *   host_interface_coh  [F * S][host_interface_slots][4][NE]: the diagonals of the specular-only versions of the same
     *                       four for mode 0 (index 2 * stream + polarisation): the coherent pass of active mode.
     * NULL host_interface_slot: every interface is Flat.  Under prune_deep_snowpack a rough interface right below the last
     * kept layer closes the recursion with its Rbot (what the reference's truncated system keeps, dort.py:443-452).  Under
     * process_coherent_layers the caller samples the matrices on the streams of the REDUCED snowpack and gives no slot to
     * an interface on top of or right below a collapsed layer (the reference's CoherentFlat takes its place,
     * interface/coherent_flat.py:37-45): the slot index stays the layer's index in the INPUT arrays. */
    const int32_t* host_interface_slot;
    const double* host_interface;
    const double* host_interface_coh;
    int32_t host_interface_slots;
    /* Wet snow (smrt/inputs/make_medium.py:316-434, smrt/permittivity/wetice.py:12-45): liquid_water [S][n_layers_max] =
     * water volume / (ice + water volume) of every layer, or NULL: dry snow.  A wet layer (> 0) must be at the melting
     * point (273.15 K: the water permittivity, Maetzler & Wegmuller 1987, is not defined below it -- status 5 otherwise);
     * its scatterers are ice spheres coated in water: permittivity by Maxwell Garnett with water as the host
     * (wetice_permittivity_bohren83, the reference's default for snow layers); frac_volume is then the volume fraction of
     * ice + water (SnowLayer.compute_frac_volumes).  Applies to the device emmodels; ignored by SMRT_EM_HOST layers. */
    const double* liquid_water;
    /* layers of kind SMRT_EM_IBA_HOST: [F * S][Lmax] the coefficient of IBA's phase matrix (see SMRT_EM_IBA_HOST), indexed
     * like host_layer by the global pair f * S + s; null when no layer has that kind */
    const double* host_iba_coeff;
    /* Rough boundaries evaluated on the device (SMRT_ROUGH_*; smrt_amd/csrc/rough_boundary_kernel.hpp): the library builds what
     * the caller of host_interface* / host_substrate* would hand over, from the layer inputs, for the pairs of the upload.
     *   rough_kind   [S][n_layers_max + 1] int32: entry l < n_layers is the interface ON TOP of layer l (0: the surface), entry
     *                n_layers the substrate; SMRT_ROUGH_NONE: not rough on the device (Flat interface; the batch's substrate_kind);
     *   rough_params [S][n_layers_max + 1][4]: geometrical_optics and geometrical_optics_backscatter: mean square slope, shadow
     *                correction (0 / 1); iem_fung92: rms height (m), correlation length (m), autocorrelation function
     *                (0 exponential, 1 gaussian), series truncation.  A NaN parameter gives the pair NaN matrices.
     * A rough substrate goes with substrate_kind = SMRT_SUBSTRATE_FLAT: substrate_p1 + i substrate_p2 is its permittivity,
     * substrate_temperature its temperature; every snowpack of the batch then has one.  Not together with host_interface_slot,
     * SMRT_SUBSTRATE_HOST or process_coherent_layers; m_max <= SMRT_ROUGH_M_MAX in active mode.  NULL rough_kind: nothing
     * of this runs. */
    const int32_t* rough_kind;
    const double* rough_params;
} smrt_batch;

/* rough_kind entries */
#define SMRT_ROUGH_NONE 0
#define SMRT_ROUGH_GEOMETRICAL_OPTICS 1            /* smrt/interface/geometrical_optics.py: bistatic reflection and transmission */
#define SMRT_ROUGH_GEOMETRICAL_OPTICS_BACKSCATTER 2 /* geometrical_optics_backscatter.py: the lobe + 1 - hemispherical reflectivity */
#define SMRT_ROUGH_IEM_FUNG92 3                    /* iem_fung92.py: Kirchhoff coherent part + the backscatter series */
#define SMRT_ROUGH_M_MAX 4                         /* largest m_max the builder is instantiated for */

/* The builder alone, for tests and tools: uploads the batch (all its pairs), builds, and copies back what the solve would read
 * -- slot [F * S][n_layers_max], itf [F * S][slots][modes][4][NE * NE], itf_coh [F * S][slots][4][NE], sub [F * S][modes][NE * NE],
 * sub_coh [F * S][modes][NE] (layouts of host_interface* / host_substrate* above; any pointer may be NULL).  The number of slots
 * is the largest count of rough interfaces in a snowpack of the batch.  Returns that number, or -1.
 * smrt_dort_rough_info: info[0] = SMRT_ROUGH_M_MAX (the capability), and of the last upload: [1] slots, [2] HIP-event time of
 * the builder kernels (ms), [3] bytes of matrices built on the device, [4] bytes of host_interface / host_substrate matrices
 * copied from the caller, [5] bytes of device memory the builder's matrices may take now (free memory plus what its buffers
 * hold already).  Returns the number of entries of the description; at most n are written. */
int32_t smrt_dort_rough_matrices(smrt_dort_ctx* ctx, const smrt_batch* batch, int32_t* slot, double* itf, double* itf_coh,
                                 double* sub, double* sub_coh);
int32_t smrt_dort_rough_info(smrt_dort_ctx* ctx, double* info, int32_t n);

/* Sizes of the output rows (doubles per pair). Passive: Tb[pol V,H][theta].  Active: I[pol][pol_inc][theta_inc]
 * with 3 x 3 polarisations V,H,U (layout of Result.data in the reference, rtsolver_utils.py:327-332). */
int32_t smrt_dort_out_stride(const smrt_batch* b);

/* Number of visible HIP devices (0 if none). */
int32_t smrt_dort_device_count(void);

/* Create / destroy a context bound to HIP device `device`.  Returns 0 on success. */
int32_t smrt_dort_create(smrt_dort_ctx** ctx, int32_t device);
void smrt_dort_destroy(smrt_dort_ctx* ctx);
const char* smrt_dort_last_error(const smrt_dort_ctx* ctx);

/*
 * One shot: H2D of the packed batch, kernel, D2H.  pair range [pair_begin, pair_begin + pair_count) of the
 * flattened list (pair_count < 0: all).  out: [pair_count][out_stride]; status: [pair_count];
 * layer_out (optional, may be NULL): [pair_count][Lmax][5] = Re eps_eff, Im eps_eff, ks, ka, n_streams;
 * stream_out (optional): [pair_count][1 + n_max_stream] = n_air, outmu[0..n_air).
 */
int32_t smrt_dort_run(smrt_dort_ctx* ctx, const smrt_batch* batch, int64_t pair_begin, int64_t pair_count,
                      double* out, int32_t* status, double* layer_out, double* stream_out);

/*
 * Sparse selection: only the listed pairs of the flattened S x F list (indices p = f * S + s, any order, repeats
 * allowed); out / status / layer_out / stream_out have n_pairs rows, row i belongs to pairs[i].  This is what a runner
 * uses when the simulations it is given are not the full Cartesian product -- a sequence of sensors zipped with a
 * sequence of snowpacks (smrt/core/model.py:505-515), or a list of (sensor, snowpack) pairs handed over one by one.
 */
int32_t smrt_dort_run_pairs(smrt_dort_ctx* ctx, const smrt_batch* batch, const int64_t* pairs, int64_t n_pairs,
                            double* out, int32_t* status, double* layer_out, double* stream_out);

/*
 * Split form for resident data and timing: upload once, launch many times, download.
 * smrt_dort_launch is asynchronous on the context's stream; smrt_dort_sync waits for it.
 * If out_dev / status_dev are non-NULL they are DEVICE pointers (e.g. torch CUDA tensors used as the send
 * buffers of an RCCL gather) that receive the results instead of the context's own buffers.
 */
int32_t smrt_dort_upload(smrt_dort_ctx* ctx, const smrt_batch* batch, int64_t pair_begin, int64_t pair_count);
int32_t smrt_dort_upload_pairs(smrt_dort_ctx* ctx, const smrt_batch* batch, const int64_t* pairs, int64_t n_pairs);
int32_t smrt_dort_launch(smrt_dort_ctx* ctx, void* out_dev, void* status_dev);
int32_t smrt_dort_sync(smrt_dort_ctx* ctx);
int32_t smrt_dort_download(smrt_dort_ctx* ctx, double* out, int32_t* status, double* layer_out,
                           double* stream_out);

/* HIP-event time (ms) of the most recent smrt_dort_launch on the context's stream (valid after sync),
 * and accumulated over all launches since the last reset (count returned through n_launches). */
double smrt_dort_last_kernel_ms(smrt_dort_ctx* ctx);

/* Per-kernel HIP-event time of the three-kernel pipelines.  enable > 0: every prep / diagonalisation / finish kernel launch
 * of the following smrt_dort_launch calls is bracketed by an event pair on its stream (a few microseconds per launch: for
 * measurement runs, not for the timed region of a benchmark); enable == 0: off; enable < 0: leave it as it is (read only).
 * ms3 != NULL: the intervals of the LAST launch summed per kind -- ms3[0] prep, [1] diagonalisation (the Jacobi launches
 * of all size classes, or the gram / tridiag / chase / vectors kernels of the symmetric eigensolver), [2] finish -- after a
 * stream synchronisation; zeros when that launch was not instrumented or the batch runs on a fused kernel.  (With several
 * concurrent pipeline passes the intervals of different passes overlap: the sums then exceed the wall time of the launch.)
 * Returns the number of intervals of the last launch, -1 on error. */
int32_t smrt_dort_kernel_breakdown(smrt_dort_ctx* ctx, int32_t enable, double* ms3);

/* How the layer eigenproblems are diagonalised on the three-kernel pipelines -- the device counterpart of the reference's
 * DORT option diagonalization_method (smrt/rtsolver/dort.py:614,821-962: eig / schur / half_rank_eig / stamnes88; all of them
 * work on the squared problem, like SMRT_DIAG_SYMMETRIC).  mode: SMRT_DIAG_JACOBI, SMRT_DIAG_SYMMETRIC (wherever it is
 * built: passive mode, streams x polarisations <= 64; other batches keep the Jacobi kernels), or -1: the default (SMRT_DIAG_SYMMETRIC;
 * the environment variable SMRT_DORT_EIG=0 / 1 overrides it for experiments).  Takes effect at the next upload. */
int32_t smrt_dort_set_diagonalisation(smrt_dort_ctx* ctx, int32_t mode);

/* The prep stage of the LDS-resident passive pipelines (streams x polarisations <= 64).  mode: SMRT_PREP_PER_PAIR (one
 * workgroup per pair works through its layers, LDS sized for the largest layer the batch may have), SMRT_PREP_PER_LAYER (a pair
 * setup kernel, then one workgroup per (pair, layer) item in one launch per size class of rows; the staging area it leaves is
 * bitwise the same), or -1: the default (the environment variable SMRT_DORT_PREP_LAYERS=0 / 1 overrides it for experiments).
 * Other batches keep their prep kernels.  Takes effect at the next upload. */
int32_t smrt_dort_set_prep(smrt_dort_ctx* ctx, int32_t mode);

/* The launches that take one size class of rows each (the per-layer prep and the symmetric eigensolver of the LDS-resident
 * passive pipelines): mode 1, over compact lists of the items of the class, built on the device at upload from the stream
 * counts of the layers (the grid of a launch is the number of its items; an empty class is not launched); 0, over every item
 * of the pipeline pass, an item of another class leaving at once; -1: the default (1; the environment variable
 * SMRT_DORT_CLASS_LISTS=0 / 1 overrides it for experiments).  The outputs are bitwise the same.  Launches in prune rounds
 * (prune_deep_snowpack) keep the full grids.  Takes effect at the next upload. */
int32_t smrt_dort_set_class_lists(smrt_dort_ctx* ctx, int32_t mode);

/* What the uploaded batch runs on, as numbers (tests assert the designed kernel choice with these instead of wall-clock
 * ratios): info[SMRT_INFO_*], at most n entries written; returns SMRT_INFO_COUNT, -1 on error.
 *   PIPELINE      SMRT_PIPELINE_*: the kernels a launch of this batch consists of
 *   CHUNK_PAIRS   pairs per pipeline pass (the staging area holds one chunk), CHUNKS: passes per launch
 *   PRUNE_ROUNDS  layer ranges the prep + Jacobi kernels run over under prune_deep_snowpack (1: all layers at once)
 *   STAGED_ITEMS  (pair, azimuth mode, layer) items the LAST chunk of the last launch diagonalised -- known when the
 *                 staging counts are reset per chunk (prune rounds, process_coherent_layers), else -1; synchronises
 *   BLOCK_THREADS workgroup size of the per-pair kernels, N_MAX: padded matrix order (streams x polarisations)
 *   DIAGONALISATION  SMRT_DIAG_*: what runs between the prep and the finish kernels of the three-kernel pipelines
 *   RAYLEIGH_CLOSED_FORM  1: the layers with a Rayleigh phase matrix (dmrt_qca_shortrange, dmrt_qcacp_shortrange,
 *                 nonscattering, rayleigh-family host emmodels) of this batch skip Cholesky and the iteration: their azimuth
 *                 mode 0 is "diagonal minus rank two" and is diagonalised in closed form (passive batches on the strip finish
 *                 kernels; SMRT_DORT_RAYLEIGH=0 switches it off for experiments)
 *   PREP          SMRT_PREP_*: the prep stage of this batch (PER_LAYER only on the LDS pipelines in passive mode)
 *   CLASS_LISTS   1: the launches per size class of rows of this batch run over item lists (smrt_dort_set_class_lists)
 *   CLASS_LIST_ITEMS  items in the lists of this upload, all classes and chunks (-1: no lists)
 *   CLASS_LIST_MISSES listed items a launch found with a staged row count of another class since the upload: always 0
 *                 (a check of the lists against the staging area; synchronises) */
enum { SMRT_INFO_PIPELINE = 0, SMRT_INFO_CHUNK_PAIRS, SMRT_INFO_CHUNKS, SMRT_INFO_PRUNE_ROUNDS, SMRT_INFO_STAGED_ITEMS,
       SMRT_INFO_BLOCK_THREADS, SMRT_INFO_N_MAX, SMRT_INFO_DIAGONALISATION, SMRT_INFO_RAYLEIGH_CLOSED_FORM, SMRT_INFO_PREP,
       SMRT_INFO_CLASS_LISTS, SMRT_INFO_CLASS_LIST_ITEMS, SMRT_INFO_CLASS_LIST_MISSES, SMRT_INFO_COUNT };
enum { SMRT_PREP_PER_PAIR = 0, SMRT_PREP_PER_LAYER = 1 };
enum { SMRT_DIAG_JACOBI = 0,      /* one-sided Jacobi on B = L+^T L- (singular values to high relative accuracy) */
       SMRT_DIAG_SYMMETRIC = 1 }; /* Householder tridiagonalisation + implicit QL on S = B B^T (passive, N <= 64: the default) */
enum { SMRT_PIPELINE_FUSED = 0,          /* one kernel per pair, matrices in LDS (N <= 64) */
       SMRT_PIPELINE_LDS_TWO_SLOT = 1,   /* prep + Jacobi + two-slot finish, matrices in LDS */
       SMRT_PIPELINE_LDS_FOUR_SLOT = 2,  /* ... with the four-slot finish kernel (set_pipeline(2)) */
       SMRT_PIPELINE_LDS_REG = 3,        /* ... with the register-resident finish kernel (passive default) */
       SMRT_PIPELINE_FUSED_GMEM = 4,     /* one kernel per pair on a global workspace (N > 64) */
       SMRT_PIPELINE_GMEM = 5,           /* prep + Jacobi + finish on the global workspace, 64 < N <= 128 */
       SMRT_PIPELINE_BIG = 6,            /* ... with the blocked Jacobi kernel, 128 < N <= 384 */
       SMRT_PIPELINE_GMEM_STRIP = 7,     /* LDS-resident prep + Jacobi + the strip finish kernel (eight wavefronts), 64 < N <= 128 (passive default) */
       SMRT_PIPELINE_LDS_STRIP = 8 };    /* prep + Jacobi + the strip finish kernel (four wavefronts), N <= 64 (passive default) */
int32_t smrt_dort_launch_info(smrt_dort_ctx* ctx, int64_t* info, int32_t n);
double smrt_dort_total_kernel_ms(smrt_dort_ctx* ctx, int64_t* n_launches, int32_t reset);

/* Tuning knob: threads per workgroup of the per-pair kernels: 64 (one wavefront) or 256 (default, also 0). */
int32_t smrt_dort_set_block_threads(smrt_dort_ctx* ctx, int32_t threads);

/* Pipeline shape.  1 (default) = three kernels -- prep per pair, Jacobi per (pair, layer[, azimuth mode]), finish per
 * pair -- with the factors staged through HBM/L2, for every size (N = streams x polarisations of the batch maximum):
 *   N <= 64:        matrices in LDS; finish = the register-resident kernel (one wavefront per pair, four per CU) in
 *                   passive mode with Flat interfaces, else the two-slot LDS kernel (two workgroups per CU);
 *   64 < N <= 128:  per-workgroup global workspace, Jacobi kernel on a 128-column LDS matrix;
 *   128 < N <= 384: global workspace, blocked Jacobi kernel (the limit of this build: n_max_stream <= 192 passive,
 *                   <= 128 active; smrt_dort_upload fails beyond).
 * In passive mode with Flat interfaces the finish kernel of 1 is the pivot-free recursion: the STRIP kernel (one workgroup
 * of four wavefronts per pair for N <= 64 while three of them share a CU, of eight for 64 < N <= 128), else the
 * register-resident one (one wavefront per pair, N <= 64).
 * 3 = like 1 with the register-resident finish kernel wherever it is supported (N <= 64) instead of the four-wavefront
 * strip kernel; 5 = like 1, the strip kernels wherever they are supported (also at two workgroups per CU); 4 = like 1,
 * never a pivot-free finish kernel (A/B runs); 2 = like 4 with the four-matrix LDS finish kernel (one workgroup per CU;
 * N <= 64 passive only, otherwise like 0); 0 = everything fused in one kernel, one workgroup per pair (no
 * prune_deep_snowpack).  Call before smrt_dort_upload.  In the environment SMRT_DORT_FINISH_REG=0|1 overrides 3 / 4 for
 * the register-resident kernel, SMRT_DORT_FINISH_STRIP=0|1 and SMRT_DORT_FINISH_STRIP4=0|1 for the two strip kernels. */
int32_t smrt_dort_set_pipeline(smrt_dort_ctx* ctx, int32_t split);

/* LDS bytes one workgroup (= one wavefront) of the register-resident finish kernel takes for a batch with this
 * n_max_stream and n_layers_max: four of them share the 160 KB of a CU while this is <= 40 KB (40 layers at 32 streams),
 * three up to 160 KB / 3 (~140 layers) -- the range in which the default pipeline takes this kernel --, two up to the
 * 64 KB a workgroup may have, where only smrt_dort_set_pipeline(ctx, 3) selects it (it ties with the two-slot kernel). */
int32_t smrt_dort_finish_reg_lds_bytes(int32_t n_max_stream, int32_t n_layers_max);

/* LDS bytes one workgroup of the strip finish kernel takes: wavefronts = 4 (N <= 64; the default pipeline takes it while
 * three workgroups share a CU, i.e. up to 160 KB / 3) or 8 (64 < N <= 128: one workgroup per CU, taken while it fits the
 * 160 KB at all).  Returns -1 for other wavefront counts. */
int32_t smrt_dort_finish_strip_lds_bytes(int32_t n_max_stream, int32_t n_layers_max, int32_t wavefronts);

/* LDS bytes one workgroup of the Jacobi kernel takes in the three-kernel pipelines of up to 128 columns (n_pol = 2
 * passive, 3 active).  The N <= 64 pipelines launch one kernel per SIZE CLASS of items (at most 32 / 33-48 / 49-56 /
 * 57-64 columns), each with the layout of its own largest item: size_class_columns = that bound, or 0 for the layout of
 * the batch maximum (the one launch of the 64 < N <= 128 pipeline).  Returns -1 for shapes outside these pipelines. */
int32_t smrt_dort_jacobi_lds_bytes(int32_t n_max_stream, int32_t n_pol, int32_t size_class_columns);

/* Algorithmic work of the uploaded batch after a launch: sum over pairs, modes and layers of N_l^3
 * (N_l = streams x polarisations in layer l), the quantity SURVEY.md 8(d) prices at 68 flops. */
double smrt_dort_sum_n3(smrt_dort_ctx* ctx);

/*
 * The emmodel protocol's ft_even_phase for ONE layer (smrt/emmodel/common.py:349-399, rayleigh.py:52-127; consumed by
 * the reference's rtsolvers at smrt/rtsolver/dort.py:231-247): azimuthal modes 0..m_max of the phase matrix on the grid
 * mu_s (scattered cosines) x mu_i (incident cosines), any signs.  out: [npol][npol][m_max + 1][n_s][n_i], npol = 2 or 3
 * (V, H[, U]).  The layer is described like a row of smrt_batch: emmodel / microstructure codes, frequency (Hz), ice
 * volume fraction, temperature (K), micro_p1 / micro_p2 (corr_length | radius, stickiness).  What lets smrt_amd's
 * emmodel classes serve an rtsolver other than smrt_amd's own DORT (which assembles these modes inside its kernels).
 */
int32_t smrt_dort_ft_even_phase(smrt_dort_ctx* ctx, int32_t emmodel, int32_t microstructure, double frequency,
                                double frac_volume, double temperature, double micro_p1, double micro_p2,
                                const double* mu_s, int32_t n_s, const double* mu_i, int32_t n_i, int32_t m_max,
                                int32_t npol, double* out);

/* Work estimate of every pair of the uploaded batch BEFORE solving it: sum over its layers (and azimuth modes) of
 * N_l^3 from the stream counts alone (a cheap kernel: layer permittivities and Snell's law only).  cost: [pair_count]
 * host doubles; 0 for a pair with invalid input.  What a caller shards by when it splits a batch over several GPUs
 * (total reflection removes streams, so the work of a pair varies with its density profile). */
int32_t smrt_dort_pair_cost(smrt_dort_ctx* ctx, double* cost);

/* Profiling builds only (-DSMRT_STAGE_TIMING): shader cycles of workgroup thread 0 per kernel stage, summed over
 * the pairs of the last launch (setup, assemble, cholesky, L^T L, jacobi, triangular, R1, LU1, R45, LU2, R78, out).
 * A regular build returns zeros. */
int32_t smrt_dort_stage_cycles(smrt_dort_ctx* ctx, double* out16);

/* Positive Gauss-Legendre nodes of order 2n in descending order (smrt/rtsolver/streams.py:300-313). Host only. */
int32_t smrt_gauss_legendre_positive(int32_t n, double* mu, double* weight);

/*
 * Multi-GPU: the (snowpack x frequency) list is embarrassingly parallel (smrt/core/model.py:395-398 maps one function
 * over it; smrt/runner/joblib_runner.py:45-72 is the reference's fan-out), so every GPU solves its own slice and the
 * ONLY communication of the path is the gather of the result rows to one rank -- done here with RCCL over xGMI,
 * device buffer to device buffer, no PyTorch involved.
 *
 * One context = one rank.  Either one process per GPU: rank 0 calls smrt_dort_comm_unique_id, the caller ships the
 * 128 bytes to the other ranks by any means it has (smrt_amd/runner/distributed.py uses a TCP socket on MASTER_ADDR),
 * every rank calls smrt_dort_comm_init (collective).  Or one process driving several GPUs: smrt_dort_comm_init_all on
 * the list of contexts (ncclCommInitAll), then smrt_dort_gather from one host thread per context.
 *
 * smrt_dort_gather (collective): the rows of the LAST launch of every rank (its own out / status buffers, i.e.
 * smrt_dort_launch(ctx, NULL, NULL)) land on `root` in rank order; counts[r] = number of pairs of rank r (the
 * caller's sharding: counts[own rank] must equal the uploaded pair count).  On the root, out [sum counts][out_stride]
 * and status [sum counts] are HOST buffers (either may be NULL to leave the rows on the device); ignored elsewhere.
 * It is enqueued on the context's stream behind the kernels and returns when the root has its rows.
 * smrt_dort_comm_allreduce_max: element-wise maximum over the ranks of n host doubles, in place (the max-over-ranks
 * of a timing; with n = 0 it is a barrier).
 * smrt_dort_comm_library: which RCCL the gather runs on -- the file the symbols were resolved from (dladdr; on failure
 * the reason) copied into path[capacity], and ncclGetVersion's code (e.g. 22703).  The environment variable
 * SMRT_RCCL_LIB pins the library (path or soname; nothing else is tried then); by default a librccl.so.1 the process
 * has already mapped is kept (it belongs to the HIP runtime in use), else /opt/rocm/lib/librccl.so.1, else the soname.
 */
#define SMRT_COMM_ID_BYTES 128
int32_t smrt_dort_comm_library(char* path, int32_t capacity, int32_t* version);
int32_t smrt_dort_comm_unique_id(char* id);
int32_t smrt_dort_comm_init(smrt_dort_ctx* ctx, int32_t world, int32_t rank, const char* id);
int32_t smrt_dort_comm_init_all(smrt_dort_ctx** ctxs, int32_t n);
int32_t smrt_dort_comm_destroy(smrt_dort_ctx* ctx);
int32_t smrt_dort_gather(smrt_dort_ctx* ctx, int32_t root, const int64_t* counts, double* out, int32_t* status);
int32_t smrt_dort_comm_allreduce_max(smrt_dort_ctx* ctx, double* values, int32_t n);

/* The transfers smrt_dort_gather issues, as data (host arithmetic only -- no GPU, no communicator): on `root` one receive
 * per other rank that has rows, the rows of rank r landing at row offset counts[0] + ... + counts[r - 1] of the gathered
 * buffer (own rows are copied to *own_offset_rows); on any other rank one send of its counts[rank] rows.  Returns the
 * number of transfers (ops beyond `capacity` are counted, not written), -1 on invalid arguments; *total_rows = sum of
 * counts.  What the multi-rank CPU tests check with 2..8 ranks, unequal and empty shards and any root. */
typedef struct smrt_gather_op { int32_t peer; int32_t reserved; int64_t offset_rows; int64_t rows; } smrt_gather_op;
int32_t smrt_dort_gather_plan(int32_t world, int32_t root, int32_t rank, const int64_t* counts, smrt_gather_op* ops,
                              int32_t capacity, int64_t* own_offset_rows, int64_t* total_rows);

/* Self-description of the ABI for foreign-function bindings: out[0] = sizeof(smrt_batch), out[1..] = byte offset of
 * every field of smrt_batch in declaration order.  Returns the number of entries of the full description (fields + 1);
 * at most `capacity` of them are written (out may be NULL to query the count).  A binding checks its own struct
 * declaration against this at load time (tests/test_host_logic.py::test_ctypes_struct_matches_the_library). */
int32_t smrt_dort_abi(int32_t* out, int32_t capacity);

const char* smrt_dort_version(void);

/*
 * The iterative first-order backscatter solver (the reference's smrt/rtsolver/iterative_first_order.py: Ulaby et al. 2014
 * eqs. 11.62, 11.74, 11.75; refraction factor of Tsang et al. 2007 eqs. 22a/b) on the same context.  Active sensors
 * only, V and H, no atmosphere.  The batch is the smrt_batch of DORT: layers, kinds, wet snow, frequencies, theta (the
 * incidence angles), the flat / reflector substrate (substrate_p1 / substrate_p2; the reflector IS allowed here) and the
 * host_layer / host_iba_coeff scalars are read; n_max_stream, m_max, phase_normalization, prune_optical_depth,
 * process_coherent_layers, the atmosphere, substrate_temperature, host_streams / host_phase, host_substrate* and
 * host_interface* are ignored.  What this solver needs beyond it travels in the struct smrt_first_order_extras; NULL means Flat
 * interfaces everywhere and no layer of kind SMRT_EM_HOST that scatters.  All arrays are indexed by the global pair f * S + s.
 *   host_interface_slot   [F * S][n_layers_max + 1] int32, or NULL: entry l < n_layers is the interface ON TOP of layer l
 *                         (0: the surface), entry n_layers the substrate; -1 = the device evaluates it (Flat interface;
 *                         substrate_kind of the batch), k >= 0 = slot k of host_interface_values holds it;
 *   host_interface_values [F * S][n_interface_slots][n_theta][10]: the caller's interface / substrate object evaluated at
 *                         the cosine the incidence angle has in the medium ABOVE the boundary (Snell from the air):
 *                         [0..1] specular reflection V, H; [2..3] coherent transmission downwards V, H; [4..5] coherent
 *                         transmission upwards V, H (at the cosine in the medium below); [6..9] the 2 x 2 diffuse
 *                         reflection at (mu, mu, azimuth pi), row-major.  A substrate leaves [2..5] zero;
 *   host_phase_samples    [F * S][n_layers_max][n_theta][4][2][2], or NULL: for layers of kind SMRT_EM_HOST the phase
 *                         matrix (V, H; NOT divided by 4 pi) at azimuth pi for (mu_s, mu_i) = (-mu, mu), (mu, -mu),
 *                         (mu, mu), (-mu, -mu), mu the cosine of the incidence direction inside the layer.  Every other
 *                         kind has its phase function on the device (IBA family, Rayleigh family, non-scattering).
 * Outputs, one row per pair: out [4][n_theta][2][2] = the contributions order 0 (surface / interface / substrate
 * backscatter), direct volume backscatter, double bounce, reflected backscatter as intensities (their sum x 4 pi cos
 * theta is sigma0); status SMRT_OK or SMRT_ERR_INPUT (the row is NaN then); optional (may be NULL) layer_out
 * [n_layers_max][5] as DORT's (column 4 is zero: no streams), backscatter_layer [n_layers_max + 1][n_theta][2][2] = what
 * the surface (first) and every layer add, scaled by 4 pi x the cosine in the layer like the reference's other_data,
 * diag [2] = largest single scattering albedo and total optical depth of the pair.
 */
typedef struct smrt_first_order_extras {
    int32_t n_interface_slots;
    int32_t reserved;
    const int32_t* host_interface_slot;
    const double* host_interface_values;
    const double* host_phase_samples;
} smrt_first_order_extras;

/* Doubles per pair of `out`: 16 x n_theta. */
int32_t smrt_first_order_out_stride(const smrt_batch* b);
/* One shot over the listed pairs (semantics of smrt_dort_run_pairs; pairs == NULL: every pair of the batch in order,
 * n_pairs ignored). */
int32_t smrt_first_order_run_pairs(smrt_dort_ctx* ctx, const smrt_batch* batch, const smrt_first_order_extras* extras,
                                   const int64_t* pairs, int64_t n_pairs, double* out, int32_t* status, double* layer_out,
                                   double* backscatter_layer, double* diag);
/* Split form: upload once, launch (asynchronous on the context's stream) any number of times, sync, download.  The
 * upload returns when the copies are done: the caller's arrays may go away or change after it.  The optional outputs are
 * always computed on the device; download copies the ones asked for (any of its pointers may be NULL).  One host thread
 * per context, as for DORT. */
int32_t smrt_first_order_upload_pairs(smrt_dort_ctx* ctx, const smrt_batch* batch, const smrt_first_order_extras* extras,
                                      const int64_t* pairs, int64_t n_pairs);
int32_t smrt_first_order_launch(smrt_dort_ctx* ctx);
int32_t smrt_first_order_sync(smrt_dort_ctx* ctx);
int32_t smrt_first_order_download(smrt_dort_ctx* ctx, double* out, int32_t* status, double* layer_out,
                                  double* backscatter_layer, double* diag);
/* HIP-event time (ms) of the two kernels of the last launch, after a sync: ms2[0] the per-(pair, layer) kernel, ms2[1]
 * the per-(pair, angle) kernel. */
int32_t smrt_first_order_kernel_ms(smrt_dort_ctx* ctx, double* ms2);
/* Self-description of smrt_first_order_extras, like smrt_dort_abi: out[0] = its size, out[1..] = the field offsets. */
int32_t smrt_first_order_abi(int32_t* out, int32_t capacity);

/*
 * The iterative second-order backscatter solver (the reference's smrt/rtsolver/iterative_second_order.py: Karam et al. 1995
 * eqs. A8, A11, A13) on the same context: the first-order solver above plus double scattering inside a layer, volume
 * scattering combined with the diffuse reflection of the substrate, and (optionally) double scattering between two layers.
 * Active sensors only, V and H, no atmosphere.  Of the smrt_batch it reads what the first-order solver reads, plus
 * n_max_stream (2 to 1024: the quadrature cosines per layer, stream_mode "most_refringent") and m_max (1 to 8: azimuth modes
 * 0 .. m_max - 1 are summed, and m_max sets the number of azimuth samples of the IBA phase function, as in the reference);
 * everything the first-order solver ignores is ignored.  Layers of kind SMRT_EM_HOST are refused.  An upload replaces the
 * resident batch of the first-order solver on this context.  The struct smrt_second_order_extras may be NULL (no interlayer
 * term, default budget, Flat interfaces, a substrate without diffuse reflection); arrays are indexed by the global pair
 * f * S + s.
 *   compute_scattering_interlayer  0 / 1: the O(L^2) interlayer term; its kernel is launched only when set;
 *   workspace_budget_bytes   everything this solver reserves beyond the first-order buffers stays inside it (<= 0: 8 GiB):
 *                            outputs, the carry, the substrate modes and, per chunk of pairs, stream sets and integrals
 *                            (n_layers_max x n_theta x (2 + n_layers_max with the interlayer term) x 4 doubles per pair).
 *                            The launch solves chunk after chunk; a budget smaller than the fixed buffers plus one pair
 *                            fails the upload;
 *   first_order              the first-order extras (host-evaluated interfaces / substrate), or NULL.  Only Flat or
 *                            Transparent inner interfaces are meaningful: this solver has no term for diffuse reflection
 *                            at an inner interface;
 *   substrate_diffuse_modes  [F * S][n_layers_max][n_theta][n_max_stream][m_max][2][2][3], or NULL (no diffuse reflection
 *                            at the substrate): for layer l, incidence angle t (cosine mu in the layer), the layer's j-th
 *                            stream cosine mu' in ASCENDING order (entries past the layer's stream count are not read) and
 *                            azimuth mode m, rows V, H (3 columns V, H, U) of the substrate's ft_even_diffuse_reflection_matrix
 *                            (3 polarisations, already over 4 pi) at [0]: (scattered -mu, incident mu') and [1]: (scattered
 *                            mu', incident mu), evaluated with the permittivity of the LAST layer, as the reference does.
 * Outputs, one row per pair: out [7][n_theta][2][2] = the four first-order contributions (bit-identical to
 * smrt_first_order_*), then order2_intralayer_scattering, order2_rough_layer_scattering, order2_interlayer_scattering;
 * status; optional layer_out and diag as the first-order solver's; backscatter_layer [n_layers_max + 1][n_theta][2][2] =
 * order 1 + order 2 per layer as the reference sums them (the order-2 part of a layer is the running sum of the two
 * non-interlayer terms down to it, times 4 pi x its cosine).
 */
typedef struct smrt_second_order_extras {
    int32_t compute_scattering_interlayer;
    int32_t reserved;
    int64_t workspace_budget_bytes;
    const smrt_first_order_extras* first_order;
    const double* substrate_diffuse_modes;
} smrt_second_order_extras;

/* Doubles per pair of `out`: 28 x n_theta. */
int32_t smrt_second_order_out_stride(const smrt_batch* b);
/* One shot over the listed pairs (semantics of smrt_dort_run_pairs; pairs == NULL: every pair of the batch in order,
 * n_pairs ignored). */
int32_t smrt_second_order_run_pairs(smrt_dort_ctx* ctx, const smrt_batch* batch, const smrt_second_order_extras* extras,
                                    const int64_t* pairs, int64_t n_pairs, double* out, int32_t* status, double* layer_out,
                                    double* backscatter_layer, double* diag);
/* Split form, as smrt_first_order_*: upload once, launch (asynchronous) any number of times, sync, download (any pointer may
 * be NULL). */
int32_t smrt_second_order_upload_pairs(smrt_dort_ctx* ctx, const smrt_batch* batch, const smrt_second_order_extras* extras,
                                       const int64_t* pairs, int64_t n_pairs);
int32_t smrt_second_order_launch(smrt_dort_ctx* ctx);
int32_t smrt_second_order_sync(smrt_dort_ctx* ctx);
int32_t smrt_second_order_download(smrt_dort_ctx* ctx, double* out, int32_t* status, double* layer_out,
                                   double* backscatter_layer, double* diag);
/* HIP-event time (ms) of the last launch, after a sync: ms2[0] the two first-order kernels, ms2[1] the order-2 kernels
 * (stream sets, integrals, walk) of every chunk. */
int32_t smrt_second_order_kernel_ms(smrt_dort_ctx* ctx, double* ms2);
/* Self-description of smrt_second_order_extras, like smrt_dort_abi: out[0] = its size, out[1..] = the field offsets. */
int32_t smrt_second_order_abi(int32_t* out, int32_t capacity);

/*
 * The successive-order-of-scattering solver (the reference's smrt/rtsolver/successive_order.py: Lenoble et al. 2007 eq. 66,
 * Greenwald et al. 2005 eq. 2) on the same context.  Passive sensors only, Flat interfaces, no atmosphere, emmodels with a
 * device implementation.  The batch is the smrt_batch of DORT: layers, kinds, wet snow, frequencies, theta, n_max_stream
 * (2 to 64), rayleigh_jeans, the flat / reflector substrate with its temperature (its own emission (1 - R) B(T) enters order
 * 0) are read; m_max only sets the number of azimuth samples of the phase function, as in the reference;
 * phase_normalization and prune_optical_depth are ignored; an atmosphere, host_* arrays, process_coherent_layers and layer
 * kinds evaluated by the caller are refused.  No new struct: the two options of the solver are arguments.
 *   n_iteration_max     orders computed at most (order 0 = emission alone);
 *   relative_tolerance  the loop stops after storing the first order whose largest emerging radiance (air streams, V and
 *                       H) is below relative_tolerance x that of order 0; later orders are exactly 0;
 *   workspace_budget_bytes  everything the solver reserves on the device for this batch stays inside it (<= 0: 8 GiB):
 *                       inputs, per-layer tables, outputs, and per chunk of pairs the weighted phase matrices
 *                       (n_layers_max x (16-padded 4 n_max_stream)^2 doubles per pair) and the workspace (radiance
 *                       profile and source: (2 K + L) x padded directions per pair, K its sublayers).  The launch solves
 *                       chunk after chunk.  A pair that does not fit alone gets SMRT_ERR_DEPTH; a budget smaller than
 *                       the buffers of the batch itself fails the upload.
 * Outputs, one row per pair: out [n_iteration_max + 1][2][n_theta] kelvin (V, H): every order through the inverse Planck
 * function by itself, last the total = inverse Planck of the summed radiances; status SMRT_OK, SMRT_ERR_INPUT or
 * SMRT_ERR_DEPTH (the row is NaN then); optional (may be NULL) layer_out [n_layers_max][5] and streams [1 + n_max_stream] as
 * DORT's, sublayers [n_layers_max] int32, max_radiance [n_iteration_max] (largest emerging radiance of every order run, 0
 * after the stop), orders [1] int32 (orders run).
 */
#define SMRT_ERR_DEPTH 7
/* Doubles per pair of `out`: (n_iteration_max + 1) x 2 x n_theta. */
int32_t smrt_successive_order_out_stride(const smrt_batch* b, int32_t n_iteration_max);
/* One shot over the listed pairs (semantics of smrt_dort_run_pairs; pairs == NULL: every pair of the batch in order,
 * n_pairs ignored). */
int32_t smrt_successive_order_run_pairs(smrt_dort_ctx* ctx, const smrt_batch* batch, int32_t n_iteration_max,
                                        double relative_tolerance, int64_t workspace_budget_bytes, const int64_t* pairs,
                                        int64_t n_pairs, double* out, int32_t* status, double* layer_out, double* streams,
                                        int32_t* sublayers, double* max_radiance, int32_t* orders);
/* Split form: upload once, launch any number of times, sync, download.  The upload returns when the copies are done.  The
 * launch reads the sublayer counts back after its first kernel (they size the chunks) and is asynchronous from there on.
 * One host thread per context, as for DORT. */
int32_t smrt_successive_order_upload_pairs(smrt_dort_ctx* ctx, const smrt_batch* batch, int32_t n_iteration_max,
                                           double relative_tolerance, int64_t workspace_budget_bytes, const int64_t* pairs,
                                           int64_t n_pairs);
int32_t smrt_successive_order_launch(smrt_dort_ctx* ctx);
int32_t smrt_successive_order_sync(smrt_dort_ctx* ctx);
int32_t smrt_successive_order_download(smrt_dort_ctx* ctx, double* out, int32_t* status, double* layer_out, double* streams,
                                       int32_t* sublayers, double* max_radiance, int32_t* orders);
/* HIP-event time (ms) of the last launch, after a sync: ms2[0] the two preparation kernels, ms2[1] the sweep kernel, each
 * summed over the chunks. */
int32_t smrt_successive_order_kernel_ms(smrt_dort_ctx* ctx, double* ms2);
/* The last launch: info[0] = chunks, info[1] = bytes reserved (all buffers), info[2] = pairs over the budget, info[3] = the
 * budget.  Returns the number of entries; at most `capacity` are written. */
int32_t smrt_successive_order_launch_info(smrt_dort_ctx* ctx, int64_t* info, int32_t capacity);

/*
 * The successive-order BACKSCATTER solver: the same method in active mode (the active branches of the reference's
 * smrt/rtsolver/successive_order.py), backscatter order by order on DORT's discrete ordinates with three polarisations (V, H,
 * U).  The batch is the smrt_batch of DORT with mode SMRT_MODE_ACTIVE: layers, kinds, wet snow, frequencies, n_max_stream (2
 * to 64), phi and the flat substrate (reflection only) are read; its theta, n_theta and m_max are NOT: the incidence angles
 * and the number of azimuth modes are arguments.  A reflector substrate (no third Stokes component), host_* arrays,
 * process_coherent_layers and layer kinds evaluated by the caller are refused.
 *   n_iteration_max, relative_tolerance  as above; the tolerance is relative_tolerance x the largest emerging radiance of
 *                       mode 0 at order 0 and stops every mode pass by itself; the coherent pass runs every order;
 *   n_theta_inc, theta_inc  the incidence angles (rad); the incident streams are the air streams that bracket them;
 *   incident_npol       1 (V), 2 (V, H) or 3 (V, H, U) incident polarisations: columns = incident_npol x incident streams;
 *   m_max               azimuth modes 0 .. m_max (at most 2 for the Rayleigh-family emmodels);
 *   workspace_budget_bytes  as above; per pair the chunk buffer holds (m_max + 1) x n_layers_max x (16-padded 6
 *                       n_max_stream)^2 doubles of weighted phase matrices and (m_max + 2) passes x columns x ((2 K + L) x
 *                       padded directions + (2 L + 1) x 3 n_max_stream) doubles of workspace, K its sublayers, columns =
 *                       incident_npol x min(2 n_theta_inc, n_max_stream).
 * Outputs, one row per pair: out [3][3][n_theta_inc][n_iteration_max + 1] (scattered polarisation, incident polarisation,
 * angle, order; the last entry is the total) as DORT's active output; status SMRT_OK, SMRT_ERR_INPUT or SMRT_ERR_DEPTH (the
 * row is NaN then); optional (may be NULL) layer_out, streams, sublayers as above, max_radiance [m_max + 2][n_iteration_max]
 * (per pass -- the coherent pass first, then the modes -- the largest emerging radiance of every order run, NaN after the
 * stop), orders [m_max + 2] int32 (orders run per pass).
 * The prefix is smrt_so_active_, not smrt_successive_order_active_: the set of functions whose names begin with
 * smrt_successive_order_ is the passive solver's eight and is counted by the suite.
 */
/* Doubles per pair of `out`: 9 x n_theta_inc x (n_iteration_max + 1). */
int32_t smrt_so_active_out_stride(int32_t n_theta_inc, int32_t n_iteration_max);
int32_t smrt_so_active_run_pairs(smrt_dort_ctx* ctx, const smrt_batch* batch, int32_t n_iteration_max,
                                               double relative_tolerance, int32_t n_theta_inc, const double* theta_inc,
                                               int32_t incident_npol, int32_t m_max, int64_t workspace_budget_bytes,
                                               const int64_t* pairs, int64_t n_pairs, double* out, int32_t* status, double* layer_out,
                                               double* streams, int32_t* sublayers, double* max_radiance, int32_t* orders);
int32_t smrt_so_active_upload_pairs(smrt_dort_ctx* ctx, const smrt_batch* batch, int32_t n_iteration_max,
                                                  double relative_tolerance, int32_t n_theta_inc, const double* theta_inc,
                                                  int32_t incident_npol, int32_t m_max, int64_t workspace_budget_bytes,
                                                  const int64_t* pairs, int64_t n_pairs);
/* As smrt_successive_order_launch, the launch is only partly asynchronous: it waits for the sublayer counts of its first
 * kernel, plans the chunks on the host from them -- again on every launch of the same upload -- and waits for the upload of
 * the workspace offsets; from there on the chunk kernels are queued without waiting. */
int32_t smrt_so_active_launch(smrt_dort_ctx* ctx);
int32_t smrt_so_active_sync(smrt_dort_ctx* ctx);
int32_t smrt_so_active_download(smrt_dort_ctx* ctx, double* out, int32_t* status, double* layer_out, double* streams,
                                              int32_t* sublayers, double* max_radiance, int32_t* orders);
/* HIP-event time (ms) of the last launch, after a sync: ms3[0] the preparation kernels, ms3[1] the sweep kernel, ms3[2] the
 * combine kernel, each summed over the chunks. */
int32_t smrt_so_active_kernel_ms(smrt_dort_ctx* ctx, double* ms3);
/* As smrt_successive_order_launch_info: returns the number of entries (>= 0), negative on error. */
int32_t smrt_so_active_launch_info(smrt_dort_ctx* ctx, int64_t* info, int32_t capacity);

/*
 * The multi-Fresnel thermal emission solver (the reference's smrt/rtsolver/multifresnel_thermalemission.py and
 * multifresnel/multifresnel.py: Hebert et al. 2015; annex of Zeiger et al. 2024) on the same context.  Passive sensors only,
 * Flat interfaces, no substrate or a Flat one, no atmosphere, emmodels with a device implementation: only their effective
 * permittivity enters the solution (ks and ka are reported).  The batch is the smrt_batch of DORT: layers, kinds, wet snow,
 * frequencies and the flat substrate with its temperature are read (the substrate becomes one more layer, 1e10 m thick);
 * theta, n_max_stream, m_max, phase_normalization, rayleigh_jeans and prune_optical_depth are ignored; an atmosphere, host_*
 * arrays and process_coherent_layers are refused.  What the solver needs beyond the batch are arguments:
 *   mu                   [n_theta] the cosines of the sensor's angles, in the air; 0 <= mu <= 1
 *   prune_deep_snowpack  the optical depth every angle starts with: the optical depth of a layer is clipped, per angle, to what
 *                        that angle has left; the chain of a pair stops after the first layer at which the remainder of the
 *                        steepest angle (largest mu) is negative;
 *   prune_none           non-zero: no pruning (the reference's None), prune_deep_snowpack is not read.
 * Per pair and angle the solution is the product, left to right, of one 2 x 3 affine matrix per layer; there is no Planck
 * function: the temperatures are the physical ones.
 * Outputs, one row per pair: out [n_theta][2] kelvin (V, H); status [n_theta] SMRT_OK, SMRT_ERR_INPUT (an invalid layer: every
 * angle of the pair) or SMRT_ERR_NONFINITE (this angle: a reflectivity of 1 divides by zero) -- the element is NaN then;
 * optional (may be NULL) layers_used [1] int32 (layer matrices multiplied, the substrate counts), tau_snowpack [1] (the steepest
 * angle's clipped optical depths summed over those layers), layer_out [n_layers_max][5] as DORT's (column 4 is zero).
 */
#define SMRT_ERR_NONFINITE 8
/* Doubles per pair of `out`: 2 x n_theta. */
int32_t smrt_multifresnel_out_stride(const smrt_batch* b);
/* One shot over the listed pairs (semantics of smrt_dort_run_pairs; pairs == NULL: every pair of the batch in order,
 * n_pairs ignored).  Returns 0, negative on error. */
int32_t smrt_multifresnel_run_pairs(smrt_dort_ctx* ctx, const smrt_batch* batch, const double* mu, double prune_deep_snowpack,
                                    int32_t prune_none, const int64_t* pairs, int64_t n_pairs, double* out, int32_t* status,
                                    int32_t* layers_used, double* tau_snowpack, double* layer_out);
/* Split form: upload once, launch (asynchronous on the context's stream) any number of times, sync, download.  The upload
 * returns when the copies are done.  One host thread per context, as for DORT. */
int32_t smrt_multifresnel_upload_pairs(smrt_dort_ctx* ctx, const smrt_batch* batch, const double* mu, double prune_deep_snowpack,
                                       int32_t prune_none, const int64_t* pairs, int64_t n_pairs);
int32_t smrt_multifresnel_launch(smrt_dort_ctx* ctx);
int32_t smrt_multifresnel_sync(smrt_dort_ctx* ctx);
int32_t smrt_multifresnel_download(smrt_dort_ctx* ctx, double* out, int32_t* status, int32_t* layers_used, double* tau_snowpack,
                                   double* layer_out);
/* HIP-event time (ms) of the two kernels of the last launch, after a sync: ms2[0] the per-(pair, layer) kernel, ms2[1] the
 * per-(pair, angle) kernel.  Returns 0, negative on error. */
int32_t smrt_multifresnel_kernel_ms(smrt_dort_ctx* ctx, double* ms2);

/*
 * The nadir LRM altimetry solver (the reference's smrt/rtsolver/nadir_lrm_altimetry.py with the Brown 1977 waveform model of
 * lrm_waveform_model.py) on the same context: the waveform of a low-rate-mode radar altimeter over a layered snowpack, first
 * order scattering, paths along the vertical.  Of the smrt_batch it reads the layers, kinds, wet snow, frequencies and the
 * scalars of layers evaluated by the caller (host_layer, host_iba_coeff); theta, the substrate fields and everything DORT-only
 * are ignored; an atmosphere, host_phase and process_coherent_layers are refused.  What one group of pairs shares is in
 * smrt_lrm_params:
 *   altitude, pulse_bandwidth, antenna_gain, nominal_gate   the sensor's;
 *   gamma            2 / ln 2 x sin^2(beamwidth / 2) of the circular antenna pattern;
 *   off_nadir_angle  radians; pulse_sigma  seconds (0.513 / pulse_bandwidth);
 *   ngate, oversampling   the waveform has ngate x oversampling sub-gates;
 *   n_mu             incidence samples of the surface / interface echo: 1 (the fast path: one convolution with the impulse
 *                    response in closed form) or theta_inc_sampling + 1 (the slow path), with their times t_inc [n_mu];
 *   shift            fast path: the index of the first sub-gate at or after the nominal gate (1 <= shift < ngate x oversampling);
 *   return_contributions  three rows (surface, interfaces, volume) instead of their sum;
 *   return_oversampled    rows of ngate x oversampling samples instead of the mean over every gate;
 *   skip_pfs_convolution  the vertical distribution itself (n_mu == 1 only);
 *   sigma_surface, surface_slope   [n_snowpacks] metres / radians, or NULL (zero); sigma_surface needs n_mu == 1;
 *   interface_values  NULL (Flat interfaces, no echo), or [n_frequencies x n_snowpacks][n_layers_max + 1][1 + n_mu] per boundary
 *                    (slot n_layers of a pair is the substrate): the one-way power transmission at nadir (NaN: Flat, evaluated on
 *                    the device; -1: transparent) and the echo per incidence sample, refraction and coherent part included.
 * At equal depth a layer boundary precedes a sub-gate.  Sub-gates beyond ngate x oversampling are not computed: none reaches an
 * output sample.
 * Outputs, one row per pair: out [rows][samples] (smrt_lrm_out_stride doubles); status [1] SMRT_OK or SMRT_ERR_INPUT (the
 * pair's outputs are NaN then); optional (may be NULL) z_gate [samples] (NaN below the snowpack), layer_out [n_layers_max][5]
 * (Re eps, Im eps, ks, ka, backward scattering / eps), vertical [1, 3 or 2 n_mu + 1][ngate x oversampling] the vertical
 * distribution before the convolution (slow path / contributions: surface rows, interface rows, volume).
 */
typedef struct smrt_lrm_params {
    double altitude;
    double pulse_bandwidth;
    double antenna_gain;
    double gamma;
    double off_nadir_angle;
    double nominal_gate;
    double pulse_sigma;
    int32_t ngate;
    int32_t oversampling;
    int32_t n_mu;
    int32_t shift;
    int32_t return_contributions;
    int32_t return_oversampled;
    int32_t skip_pfs_convolution;
    int32_t reserved;
    const double* t_inc;
    const double* sigma_surface;
    const double* surface_slope;
    const double* interface_values;
} smrt_lrm_params;
/* Doubles per pair of `out`. */
int32_t smrt_lrm_out_stride(const smrt_lrm_params* p);
/* One shot over the listed pairs (semantics of smrt_dort_run_pairs; pairs == NULL: every pair of the batch in order,
 * n_pairs ignored).  Returns 0, negative on error. */
int32_t smrt_lrm_run_pairs(smrt_dort_ctx* ctx, const smrt_batch* batch, const smrt_lrm_params* params, const int64_t* pairs,
                           int64_t n_pairs, double* out, int32_t* status, double* z_gate, double* layer_out, double* vertical);
/* Split form: upload once, launch (asynchronous on the context's stream) any number of times, sync, download. */
int32_t smrt_lrm_upload_pairs(smrt_dort_ctx* ctx, const smrt_batch* batch, const smrt_lrm_params* params, const int64_t* pairs,
                              int64_t n_pairs);
int32_t smrt_lrm_launch(smrt_dort_ctx* ctx);
int32_t smrt_lrm_sync(smrt_dort_ctx* ctx);
/* The layer scalars of the uploaded batch alone: runs the (pair, layer) kernel and copies layer_out [pairs][n_layers_max][5],
 * synchronously.  It is how a caller that evaluates interfaces on the host gets the permittivities it needs, before the upload
 * that carries interface_values. */
int32_t smrt_lrm_layers(smrt_dort_ctx* ctx, double* layer_out);
int32_t smrt_lrm_download(smrt_dort_ctx* ctx, double* out, int32_t* status, double* z_gate, double* layer_out, double* vertical);
/* HIP-event time (ms) of the three kernels of the last launch, after a sync: layer scalars, vertical distribution, waveform. */
int32_t smrt_lrm_kernel_ms(smrt_dort_ctx* ctx, double* ms3);
/* [sizeof(smrt_lrm_params), offset of every field in declaration order] as compiled; returns the number of entries. */
int32_t smrt_lrm_abi(int32_t* out, int32_t capacity);

/*
 * The nadir SAR altimetry solver (the reference's smrt/rtsolver/nadir_sar_altimetry.py with the Dinardo et al. 2018 delay-Doppler
 * model of delay_doppler_model/dinardo18.py) on the same context: the delay-Doppler map of a SAR altimeter over a layered
 * snowpack.  It reads of the smrt_batch what the LRM solver reads, and takes ONE frequency per batch.  What one group of pairs
 * shares is in smrt_sar_params:
 *   altitude, pulse_bandwidth, nominal_gate, pulse_repetition_frequency, wavelength, velocity, alpha   the sensor's;
 *   pitch_angle, roll_angle   radians;
 *   sigma_p, theta_lim, gamma_x, gamma_y, l_gamma, lz, pu   the constants of the model (D18 eq. 18, 19, 27; R15 eq. 37);
 *   nu_coherent      one over the square decay of the coherent reflection (Fung and Eom 1983);
 *   ngate, ndoppler, oversampling_time, oversampling_doppler   the oversampled map has ngate x oversampling_time delays and
 *                    ndoppler x oversampling_doppler Doppler frequencies (ndoppler even);
 *   return_oversampled   the oversampled map instead of the mean over every oversampling block;
 *   n_rows           output rows per pair;
 *   n_tables, table_sigma [n_tables], table_index [n_snowpacks]   the distinct sigma_surface (metres) and the one of every snowpack;
 *   boundary_values  [n_snowpacks][n_layers_max + 1][4] per boundary (slot n_layers of a snowpack is the substrate): the one-way
 *                    power transmission at nadir (NaN: Flat, on the device; -1: transparent), the coherent and the incoherent
 *                    echo before attenuation, one over the mean square slope (0 where the incoherent echo is 0);
 *   row_map          [n_snowpacks][2 (n_layers_max + 1) + 2] the output row (or -1) of the incoherent echo of every boundary, of the
 *                    coherent echo of every boundary and of the volume; then the row of the total, which takes every source.
 * Outputs, one row per pair: out [n_rows][delays][Doppler frequencies] (smrt_sar_out_stride doubles); status [1] SMRT_OK or
 * SMRT_ERR_INPUT (invalid layers, or a boundary with a positive echo later than the window: the map is NaN then); optional
 * (may be NULL) z_gate [delays] (NaN below the snowpack), layer_out [n_layers_max][5] as the LRM solver's, vertical
 * [ngate x oversampling_time] the volume backscatter per sub-gate, echo [n_layers_max + 1][4] per boundary: two-way travel
 * time, attenuated coherent and incoherent echo, shift in samples.  The maps of one launch stay below 2 GiB: more pairs are refused.
 *
 * Appended for the delay-Doppler model of Halimi et al. 2014 (delay_doppler_model/halimi14.py); a caller that zero-fills the
 * struct gets Dinardo18:
 *   delay_doppler_model      SMRT_SAR_DINARDO18 (0) or SMRT_SAR_HALIMI14 (1); any other value is refused;
 *   slant_range_correction   Halimi14: the delay compensation per Doppler column (0: the pseudo-LRM mode);
 *   delay_window_widening    Halimi14: the impulse response and the convolutions are made on ngate x delay_window_widening
 *                            gates, of which the first ngate are kept (>= 1 then; Dinardo18 reads none of the three);
 *   h14_pu, h14_gamma, burst_duration   Halimi14: Pu x ndoppler^2 (H14 after eq. 3, in the Nb^2 convention of eq. 14), gamma
 *                            of the mean of the two beamwidths (after eq. 3), the duration of a burst (eq. 19).
 * With Halimi14 a group has ONE table per distinct sigma_surface and every boundary adds that table, shifted and scaled by its
 * echoes: sigma_p ... nu_coherent and the fourth boundary value are not read.
 */
enum { SMRT_SAR_DINARDO18 = 0, SMRT_SAR_HALIMI14 = 1 };
typedef struct smrt_sar_params {
    double altitude;
    double pulse_bandwidth;
    double nominal_gate;
    double pulse_repetition_frequency;
    double wavelength;
    double velocity;
    double alpha;
    double pitch_angle;
    double roll_angle;
    double sigma_p;
    double theta_lim;
    double gamma_x;
    double gamma_y;
    double l_gamma;
    double lz;
    double pu;
    double nu_coherent;
    int32_t ngate;
    int32_t ndoppler;
    int32_t oversampling_time;
    int32_t oversampling_doppler;
    int32_t return_oversampled;
    int32_t n_rows;
    int32_t n_tables;
    int32_t reserved;
    const double* table_sigma;
    const int32_t* table_index;
    const double* boundary_values;
    const int32_t* row_map;
    int32_t delay_doppler_model;
    int32_t slant_range_correction;
    int32_t delay_window_widening;
    int32_t reserved2;
    double h14_pu;
    double h14_gamma;
    double burst_duration;
} smrt_sar_params;
/* Doubles per pair of `out` (negative: invalid parameters). */
int32_t smrt_sar_out_stride(const smrt_sar_params* p);
/* One shot over the listed pairs (semantics of smrt_dort_run_pairs; pairs == NULL: every pair of the batch in order,
 * n_pairs ignored).  Returns 0, negative on error. */
int32_t smrt_sar_run_pairs(smrt_dort_ctx* ctx, const smrt_batch* batch, const smrt_sar_params* params, const int64_t* pairs,
                           int64_t n_pairs, double* out, int32_t* status, double* z_gate, double* layer_out, double* vertical, double* echo);
/* Split form: upload once, launch (asynchronous on the context's stream) any number of times, sync, download. */
int32_t smrt_sar_upload_pairs(smrt_dort_ctx* ctx, const smrt_batch* batch, const smrt_sar_params* params, const int64_t* pairs,
                              int64_t n_pairs);
int32_t smrt_sar_launch(smrt_dort_ctx* ctx);
int32_t smrt_sar_sync(smrt_dort_ctx* ctx);
int32_t smrt_sar_download(smrt_dort_ctx* ctx, double* out, int32_t* status, double* z_gate, double* layer_out, double* vertical, double* echo);
/* HIP-event time (ms) of the four stages of the last launch, after a sync: layer scalars, vertical distribution and echoes,
 * tables (f0 / f1; with Halimi14 its three kernels summed), map. */
int32_t smrt_sar_kernel_ms(smrt_dort_ctx* ctx, double* ms4);
/* [sizeof(smrt_sar_params), offset of every field in declaration order] as compiled; returns the number of entries. */
int32_t smrt_sar_abi(int32_t* out, int32_t capacity);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* SMRT_DORT_H */
