* passive switch mixer: one MOSFET, driven hard by the LO, chops the RF into an RC load
Vlo g 0 SIN 1.0 1.0 1e6 0
Vrf rf 0 DC 0.5 AC 1
Rs rf d 200
M1 d g s n 20e-6 1e-6 2
RL s 0 2k
CL s 0 200p
.MODEL 2 VT 0.5 MU 3e-2 COX 6e-3 LAMBDA 0.02 CJ0 4.0e-14
.TRAN 15.625n 2u
.hb 1e6 3
.PNOISE V(s,d) Vrf LIN 3 0.3e6 0.9e6 2
