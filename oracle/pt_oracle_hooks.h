/*
 * pt_oracle_hooks.h — the CLOSED set of places where a study build may enter the contract (oracle/pt_oracle.c).
 *
 * A study build (oracle/study/pt_oracle_witness.c, oracle/study/pt_oracle_margins.c) is a translation unit that defines some of
 * these macros and then #includes pt_oracle.c.  Every hook has its identity default here; with the defaults pt_oracle.c IS the
 * contract, and nothing of a study build can reach it any other way.  A hook that is a statement may `return` from the function
 * it sits in (the alternative bodies do); a hook that is an expression is evaluated exactly where the contract evaluates it.
 *
 * The contract's types a hook's function may take by value are tagged (struct v3, rgb, HitInfo, Ctx), so that a study unit can
 * declare such functions before it includes the contract and define them after.
 */
#ifndef PT_ORACLE_HOOKS_H
#define PT_ORACLE_HOOKS_H

/* ------------------------------------------------------------------ values and decisions */
#ifndef perturbed        /* result y of primitive prim (0 rcp, 1 rsqrt, 2 sqrt, 3 sin, 4 cos, 5 exp, 6 pow5): may return it some ulps off */
#define perturbed(prim, y) (y)
#endif
#ifndef DECIDE           /* a data-dependent comparison (a - b = diff, operands of size scale): may number it, record it, invert it */
#define DECIDE(cond, diff, scale) (cond)
#endif
#ifndef FLIPPED_NONNEG   /* after DECIDE(x < 0) let the path go on: an inverted decision clamps the negative x to 0 (a grazing hit, k = 0) */
#define FLIPPED_NONNEG(x) ((void)0)
#endif
#ifndef c_fma            /* a contract multiply-add OUTSIDE the primitives (inside them the contract writes fmaf): may count it, unfuse it */
#define c_fma(a, b, c) fmaf((a), (b), (c))
#endif
#ifndef QUOT             /* a / b where the contract multiplies by the reciprocal rb it has already: may divide instead */
#define QUOT(a, b, rb) ((a) * (rb))
#endif
#ifndef MIX_OTHER_FORM   /* non-zero: mix(x, y, a) as x + a (y - x) instead of the contract's x (1 - a) + y a */
#define MIX_OTHER_FORM() 0
#endif
#ifndef SIG_NOTE         /* a discrete event of the path (object hit, lobe taken, how it ended): may hash it into a path signature */
#define SIG_NOTE(ev) ((void)0)
#endif

/* ------------------------------------------------------------------ alternative bodies, orders and filters (statements; may return) */
#ifndef ALT_PRIMITIVE    /* first statement of primitive prim(x): may return another conforming evaluation (correctly rounded, llvmpipe's) */
#define ALT_PRIMITIVE(prim, x) ((void)0)
#endif
#ifndef ALT_SINCOS       /* the same for f_sincos(a, sn, cs), which returns through its pointers */
#define ALT_SINCOS(a, sn, cs) ((void)0)
#endif
#ifndef ALT_DOT          /* first statement of v_dot(a, b): may return the three products summed in another order */
#define ALT_DOT(a, b) ((void)0)
#endif
#ifndef ALT_MAT_VEC      /* first statement of mat_vec: may fill out[4] with the four column terms summed in another order and return */
#define ALT_MAT_VEC(m, x, y, z, w, out) ((void)0)
#endif
#ifndef ALT_NAN_ENV      /* first statement of sample_env(c, d): may note a NaN direction and return a colour of its own for it */
#define ALT_NAN_ENV(d) ((void)0)
#endif
#ifndef ENV_FILTER       /* one channel of the bilinear cube filter, contract = the contract's weighted sum; corner: a tap fell off two edges.
                            May evaluate two nested lerps instead (and then must not evaluate `contract`) */
#define ENV_FILTER(corner, t00, t10, t01, t11, wu, wv, contract) ((void)(corner), (contract))
#endif
#ifndef ALT_SLABS        /* after the contract's slab distances t0s, t1s = (mn - o) * invd, (mx - o) * invd: may replace them by the literal / d */
#define ALT_SLABS(t0s, t1s, mn, mx, o, d) ((void)(d))
#endif
#ifndef ALT_NDC          /* after the contract's ndcx, ndcy (uniform 1 / W, 1 / H): may replace them by the literal / imgResultSize */
#define ALT_NDC(ndcx, ndcy, px, u0, py, u1, c) ((void)0)
#endif

/* ------------------------------------------------------------------ per-pixel state */
#ifndef PIXEL_BEGIN      /* first statement of shade_pixel: may reset per-pixel counters (last = the accumulation value, 4 floats) */
#define PIXEL_BEGIN(last) ((void)0)
#endif
#ifndef PIXEL_END        /* last statement of shade_pixel: may replace out[3] (the reference's alpha 1) by what it gathered */
#define PIXEL_END(out) ((void)0)
#endif

/* ------------------------------------------------------------------ decision margins: one hook per site, arguments = the locals it reads.
 * All are statements that compute error bounds NEXT TO the path and never change a value of it. */
#ifndef MARGIN_CUBOID_NORMAL   /* cuboid_normal: the three step(EPSILON, ...) comparisons */
#define MARGIN_CUBOID_NORMAL(mn, mx, p, cs, half) ((void)0)
#endif
#ifndef MARGIN_TRACE_LOCALS    /* ray_trace: may declare locals that remember what the final winner was compared with */
#define MARGIN_TRACE_LOCALS ((void)0)
#endif
#ifndef MARGIN_NOTE_ACCEPT     /* ray_trace: an object was accepted; T, winner = the hit it replaces, t1 = its entry distance */
#define MARGIN_NOTE_ACCEPT(T, winner, t1) ((void)0)
#endif
#ifndef MARGIN_TRACE           /* ray_trace, both loops done: the acceptance chains' margins, the hit point's error */
#define MARGIN_TRACE(c, o, d, invd, winner, T) ((void)0)
#endif
#ifndef MARGIN_REFRACT         /* f_refract: k < 0 (total internal reflection) */
#define MARGIN_REFRACT(k, eta, ni) ((void)0)
#endif
#ifndef MARGIN_LOBE            /* bsdf: the lobe selection against the roll */
#define MARGIN_LOBE(h, spec, refr, roll) ((void)0)
#endif
#ifndef MARGIN_HIT             /* radiance, after a hit (and Beer's law): the normal's and the cosine's error */
#define MARGIN_HIT(h) ((void)0)
#endif
#ifndef MARGIN_BOUNCE          /* radiance, after bsdf(): the new ray's error; the emissive term's */
#define MARGIN_BOUNCE(h, ro, throughput) ((void)0)
#endif
#ifndef MARGIN_ROULETTE        /* radiance: Russian roulette of bounce i against p (peeks at the next draw of *seed) */
#define MARGIN_ROULETTE(c, i, seed, p) ((void)0)
#endif
#ifndef MARGIN_ENV             /* radiance, the path left the scene: the environment's gradient times the direction's error */
#define MARGIN_ENV(c, rd, e, throughput) ((void)0)
#endif
#ifndef MARGIN_PRIMARY_RAY     /* shade_pixel: the primary ray's own error */
#define MARGIN_PRIMARY_RAY(ro) ((void)0)
#endif
#ifndef MARGIN_PIXEL_BEGIN     /* the drivers, before shade_pixel: reset the pixel's margin */
#define MARGIN_PIXEL_BEGIN() ((void)0)
#endif
#ifndef MARGIN_PIXEL_READ      /* the drivers, after shade_pixel: dst[0] = the pixel's smallest margin, dst[1] = its flip-free error per unit eps */
#define MARGIN_PIXEL_READ(dst, spp) ((dst)[0] = INFINITY, (dst)[1] = 0.0f)
#endif

/* ------------------------------------------------------------------ entry points
 * Every library exports every pto_* symbol.  A study unit that implements its entry points says so; pt_oracle.c ends with the stubs
 * (return -1) of the ones no unit of the build implements. */
/* #define PTO_HAVE_WITNESS_ENTRY_POINTS    pto_set_perturbation ... pto_witness_search are defined by the including unit */
/* #define PTO_HAVE_MARGINS_ENTRY_POINTS    pto_render_frame_margins is defined by the including unit */

#endif
